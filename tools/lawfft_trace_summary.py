#!/usr/bin/env python3
"""tools/gfisrv2_trace_summary.py for a trace of tools/lawfft_frame_time.py: the same table, with the LAWFFT entry points among those that
get their achieved TB/s (and TFLOP/s, where the plan prices their FLOP) from the plan's models.
usage: lawfft_trace_summary.py KERNEL_TRACE.csv OUT.csv LABELS.json"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gfisrv2_trace_summary as T  # noqa: E402

T.GROUPS = (('rsa_gfisr_dft', 'gfisr_dft'), ('rsa_lawfft_wincorr', 'lf_wincorr_kernel'), ('rsa_lawfft_spec_mul', 'lf_spec_mul_kernel'), ('rsa_lawfft_norm_mul', 'lf_norm_mul_kernel'),
            ('rsa_lawfft_kernel_gen', 'lf_pool_kernel'), ('rsa_lawfft_dyn_dwconv', 'lf_dyn_dwconv_kernel'), ('rsa_eimn_sal', 'eimn_sal'), ('rsa_dwconv3x3', 'dwconv3x3'))  # fmt: skip

if __name__ == '__main__':
    T.main()
