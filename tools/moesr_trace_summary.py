#!/usr/bin/env python3
"""Per-launch medians from a rocprofv3 kernel trace (``--kernel-trace --output-format csv``) of tools/moesr_frame_time.py.

With LABELS.json (``moesr_frame_time.py --labels``): the rsa_moesr_stream dispatches are taken in trace order, one forward after the other
(every forward launches the same list), so dispatch i of a forward is launch i of the plan; the output has one row per kind of launch with
the count per forward, the median time and the achieved bytes/s against the kernel's byte model.  Without it: one row per kernel name
containing any of the given substrings (the MoSRv2 pair: ``gn_apply_kernel`` ``layernorm_regs_kernel``).
usage: moesr_trace_summary.py KERNEL_TRACE.csv OUT.csv LABELS.json | NAME_SUBSTRING..."""
import csv
import json
import statistics
import sys


def main():
    trace, out, rest = sys.argv[1], sys.argv[2], sys.argv[3:]
    with open(trace, newline='') as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    dur = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3  # noqa: E731  (us)
    with open(out, 'w', newline='') as f:
        w = csv.writer(f)
        if rest and rest[0].endswith('.json'):
            with open(rest[0]) as lf:
                lab = json.load(lf)
            launches = lab['launches']
            d = [r for r in rows if 'moesr_stream_kernel' in r['Kernel_Name']]
            if len(d) != lab['forwards'] * len(launches):
                raise SystemExit(f'{len(d)} dispatches in the trace, {lab["forwards"]} forwards of {len(launches)} launches expected')
            kinds: dict = {}
            for i, r in enumerate(d):
                if i < 2 * len(launches):
                    continue  # the two warm-up forwards
                L = launches[i % len(launches)]
                kinds.setdefault((L['label'], L['bytes']), []).append(dur(r))
            w.writerow(['launch', 'per_forward', 'median_us', 'min_us', 'model_bytes', 'achieved_TB_per_s'])
            for (label, nbytes), t in kinds.items():
                med = statistics.median(t)
                w.writerow([label, len(t) // (lab['forwards'] - 2), f'{med:.2f}', f'{min(t):.2f}', nbytes, f'{nbytes / med / 1e6:.3f}'])
        else:
            w.writerow(['kernel_name_contains', 'dispatches', 'median_us', 'min_us', 'total_us'])
            for sub in rest:
                t = [dur(r) for r in rows if sub in r['Kernel_Name']]
                w.writerow([sub, len(t), f'{statistics.median(t):.2f}', f'{min(t):.2f}', f'{sum(t):.1f}'])
            t = [dur(r) for r in rows]
            w.writerow(['(every kernel)', len(t), f'{statistics.median(t):.2f}', f'{min(t):.2f}', f'{sum(t):.1f}'])
    print(open(out).read())


if __name__ == '__main__':
    main()
