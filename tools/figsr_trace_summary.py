#!/usr/bin/env python3
"""tools/gfisrv2_trace_summary.py for a trace of tools/figsr_frame_time.py: the same table, with rsa_figsr_mix among the entry points
that get their achieved TB/s from the plan's byte model.
usage: figsr_trace_summary.py KERNEL_TRACE.csv OUT.csv LABELS.json"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gfisrv2_trace_summary as T  # noqa: E402

T.GROUPS = T.GROUPS + (('rsa_figsr_mix', 'figsr_mix_kernel'),)

if __name__ == '__main__':
    T.main()
