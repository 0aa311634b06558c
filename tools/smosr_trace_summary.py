#!/usr/bin/env python3
"""Per-launch medians of rsa_smosr_gate and rsa_smosr_pa from a rocprofv3 kernel trace (``--kernel-trace --output-format csv``) of
tools/smosr_frame_time.py, with its LABELS.json: the dispatches of either kernel are taken in trace order, one forward after the other
(every forward launches the same list), so dispatch i of a forward is launch i of the plan.  One row per kind of launch: the count per
forward, the median time and the achieved bytes/s against the kernel's byte model.  For a gate launch the three dispatches in front of it
are its block's convolutions (the plan emits body.0, body.2, body.4, gate), so the row also gives the gate's share of its SMB.
usage: smosr_trace_summary.py KERNEL_TRACE.csv OUT.csv LABELS.json"""
import csv
import json
import statistics
import sys


def main():
    trace, out, labels = sys.argv[1:4]
    with open(trace, newline='') as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    with open(labels) as f:
        lab = json.load(f)
    dur = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3  # noqa: E731  (us)
    launches = lab['launches']
    ours = [i for i, r in enumerate(rows) if 'smosr_gate_kernel' in r['Kernel_Name'] or 'smosr_pa_kernel' in r['Kernel_Name']]
    if len(ours) != lab['forwards'] * len(launches):
        raise SystemExit(f'{len(ours)} dispatches in the trace, {lab["forwards"]} forwards of {len(launches)} launches expected')
    kinds: dict = {}
    for j, i in enumerate(ours):
        if j < lab['warmup'] * len(launches):
            continue
        L = launches[j % len(launches)]
        t, smb = dur(rows[i]), None
        if L['kernel'] == 'rsa_smosr_gate':
            smb = t + sum(dur(r) for r in rows[i - 3 : i])
        kinds.setdefault((L['kernel'], L['label'], L['bytes']), []).append((t, smb))
    timed = lab['forwards'] - lab['warmup']
    with open(out, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['kernel', 'launch', 'per_forward', 'median_us', 'min_us', 'model_bytes', 'achieved_TB_per_s', 'median_share_of_its_SMB'])
        for (kernel, label, nbytes), ts in kinds.items():
            t = [a for a, _ in ts]
            med = statistics.median(t)
            share = '' if ts[0][1] is None else f'{statistics.median(a / b for a, b in ts):.3f}'
            w.writerow([kernel, label, len(t) // timed, f'{med:.2f}', f'{min(t):.2f}', nbytes, f'{nbytes / med / 1e6:.3f}', share])
    print(open(out).read())


if __name__ == '__main__':
    main()
