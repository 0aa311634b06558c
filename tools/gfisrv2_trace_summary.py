#!/usr/bin/env python3
"""Per-kernel time per frame from a rocprofv3 kernel trace (``--kernel-trace --output-format csv``) of tools/gfisrv2_frame_time.py, with
its LABELS.json: the dispatches after the warm-up forwards are summed per kernel name and divided by the timed forwards.  One row per
kernel name: dispatches and microseconds per frame and the share of the frame's kernel time; the GFISR kernels (rsa_gfisr_dft's four
passes together, rsa_gfisr_spectral, the gate) also get their achieved TFLOP/s (against the 157 TF f32-MFMA peak) and TB/s from the FLOP
and byte models the plan attached to their launches.
usage: gfisrv2_trace_summary.py KERNEL_TRACE.csv OUT.csv LABELS.json"""
import csv
import json
import re
import sys

GROUPS = (('rsa_gfisr_dft', 'gfisr_dft'), ('rsa_gfisr_spectral', 'gfisr_spectral'), ('rsa_gfisr_gate', 'gated_dwconv_kernel'), ('rsa_gated_dwconv', 'gated_dwconv_kernel'))
PEAK_F32_MFMA = 157.3e12


def main():
    trace, out, labels = sys.argv[1:4]
    with open(trace, newline='') as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r['Start_Timestamp']))
    with open(labels) as f:
        lab = json.load(f)
    timed = lab['forwards'] - lab['warmup']
    # the timed forwards are the tail of the trace: every forward launches the same list
    names: dict = {}
    by_name: dict = {}
    for r in rows:
        by_name.setdefault(r['Kernel_Name'], []).append(r)
    for name, mine in by_name.items():
        k = len(mine) // lab['forwards']  # dispatches per forward (a kernel that also runs at pack time keeps its tail)
        if k == 0:
            continue
        tail = mine[len(mine) - k * timed :]
        us = sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in tail) / 1e3 / timed
        names[name] = (k, us)
    total = sum(us for _, us in names.values())
    short = lambda s: re.sub(r'\s+', ' ', s)[:110]  # noqa: E731
    with open(out, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['kernel', 'dispatches_per_frame', 'us_per_frame', 'share_of_kernel_time', 'model_TFLOP_per_frame', 'achieved_TFLOP_per_s', 'of_f32_mfma_peak',
                    'model_GB_per_frame', 'achieved_TB_per_s'])  # fmt: skip
        for name, (k, us) in sorted(names.items(), key=lambda kv: -kv[1][1]):
            w.writerow([short(name), k, f'{us:.1f}', f'{us / total:.4f}', '', '', '', '', ''])
        for entry, needle in GROUPS:
            if entry not in lab['kernels']:
                continue
            model = lab['kernels'][entry]
            k = sum(v[0] for n, v in names.items() if needle in n)
            us = sum(v[1] for n, v in names.items() if needle in n)
            if not us:
                continue
            flop, nbytes = model['flop'], model['bytes']
            w.writerow([f'{entry} (all passes)', k, f'{us:.1f}', f'{us / total:.4f}', f'{flop / 1e12:.4f}' if flop else '', f'{flop / us / 1e6:.2f}' if flop else '',
                        f'{flop / us * 1e6 / PEAK_F32_MFMA:.4f}' if flop else '', f'{nbytes / 1e9:.4f}', f'{nbytes / us / 1e6:.3f}'])  # fmt: skip
        w.writerow(['total kernel time', int(sum(k for k, _ in names.values())), f'{total:.1f}', '1.0000', '', '', '', '', ''])
    print(open(out).read())


if __name__ == '__main__':
    main()
