#!/usr/bin/env python3
"""Secondary BASELINE.json configs (C3 SPANPlus, C4 SwinIR-L, plus SPAN and the other built families) on one MI355X: one JSON line per config.

The headline config (C2, RRDBNet-23 1080p) is bench.py; this script reports the other rows of SURVEY.md §8d with the same
conventions (input resident in HBM, synchronised, median of `--reps` after warm-up).
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import resselt_amd  # noqa: E402
from resselt_amd.utils import synth  # noqa: E402


def timed(model, x, reps, warm=2):
    for _ in range(warm):
        model(x)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        y = model(x)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return y, statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    cases = {
        'C3_spanplus_x4_ps_fp16_b8_512': (synth.spanplus_state_dict(upscale=4, upsampler='ps'), (8, 3, 512, 512), torch.float16, 53_154, 276),
        'C3_spanplus_x4_dys_fp16_b8_512': (synth.spanplus_state_dict(upscale=4, upsampler='dys'), (8, 3, 512, 512), torch.float16, None, None),
        'span_x4_fp16_b8_512': (synth.span_state_dict(upscale=4), (8, 3, 512, 512), torch.float16, 53_154, 276),
        'C4_swinir_L_x4_bf16_1024': (
            synth.swinir_state_dict(embed_dim=240, depths=[6] * 9, num_heads=[8] * 9, upscale=4, upsampler='nearest+conv', resi='3conv'),
            (1, 3, 1024, 1024), torch.bfloat16, 3_833_694, 27_600),
        # SURVEY.md §8 a17 (no BASELINE config): the published DAT x4 (embed 180, 6 groups x 6 blocks, 6 heads, split 8x32, expansion 4)
        'dat_x4_bf16_512': (
            synth.dat_state_dict(embed_dim=180, depth=(6,) * 6, num_heads=(6,) * 6, split_size=(8, 32), expansion_factor=4.0, upscale=4, img_size=64),
            (1, 3, 512, 512), torch.bfloat16, None, None),
        # HAT x4 at its published size (embed 180, 6 groups x 6 blocks, 6 heads, window 16, overlap 0.5, mlp 2)
        'hat_x4_bf16_512': (
            synth.hat_state_dict(embed_dim=180, depths=(6,) * 6, num_heads=(6,) * 6, window=16, upscale=4, mlp_ratio=2.0),
            (1, 3, 512, 512), torch.bfloat16, None, None),
        # DRCT x4 at its published size (embed 180, 6 dense groups, 6 heads, window 16, gc 32, mlp 2)
        'drct_x4_bf16_512': (synth.drct_state_dict(num_layers=6, upscale=4), (1, 3, 512, 512), torch.bfloat16, None, None),
        # RGT / RGT-S x4 from the paper (embed 180, 8 / 6 groups x 6 blocks, 6 heads, mlp 2, split 8x32, c_ratio 0.5); 512^2 = 1,024 pooled keys
        'rgt_x4_bf16_512': (
            synth.rgt_state_dict(embed_dim=180, depth=(6,) * 8, num_heads=(6,) * 8, split_size=(8, 32), mlp_ratio=2.0, upscale=4, c_ratio=0.5),
            (1, 3, 512, 512), torch.bfloat16, None, None),
        'rgt_s_x4_bf16_512': (
            synth.rgt_state_dict(embed_dim=180, depth=(6,) * 6, num_heads=(6,) * 6, split_size=(8, 32), mlp_ratio=2.0, upscale=4, c_ratio=0.5),
            (1, 3, 512, 512), torch.bfloat16, None, None),
        # FDAT x4 with the reference constructor's defaults (embed 120, 4 groups x 3 x [spatial, channel], 4 heads, window 8, ffn 2, AIM 8,
        # transpose+conv), and the same trunk with the lda head (mid 64), whose two kernels run at the 2048^2 output resolution
        'fdat_x4_bf16_512': (synth.fdat_state_dict(embed_dim=120, num_groups=4, depth_per_group=3, num_heads=4, window_size=8, mid_dim=64, scale=4),
                             (1, 3, 512, 512), torch.bfloat16, None, None),
        'fdat_x4_lda_bf16_512': (synth.fdat_state_dict(embed_dim=120, num_groups=4, depth_per_group=3, num_heads=4, window_size=8, mid_dim=64, scale=4,
                                                       upsampler_type='lda'), (1, 3, 512, 512), torch.bfloat16, None, None),
        # OmniSR x4 with the common checkpoint shape (num_feat 64, res_num 5, block_num 1, window 8, pe)
        'omnisr_x4_bf16_512': (synth.omnisr_state_dict(num_feat=64, res_num=5, block_num=1, pe=True, window_size=8, up_scale=4),
                               (1, 3, 512, 512), torch.bfloat16, None, None),
        # ATD-light x4 (embed 48, 4 blocks x 6 layers, 4 heads, window 16, 64 tokens, category_size 128) and ATD x4 at its released width
        # (embed 210, 6 blocks x 6 layers, 6 heads, window 16, 128 tokens of width 10, category_size 256), both at 256^2: the f32 sim map is
        # n * m * 4 bytes per image (16.8 MB / 33.5 MB here)
        'atd_light_x4_bf16_256': (synth.atd_state_dict(embed_dim=48, depths=(6,) * 4, num_heads=(4,) * 4, window_size=16, num_tokens=64, reducted_dim=8,
                                                       mlp_ratio=1.0, upscale=4, upsampler='pixelshuffledirect'), (1, 3, 256, 256), torch.bfloat16, None, None),
        'atd_x4_bf16_256': (synth.atd_state_dict(embed_dim=210, depths=(6,) * 6, num_heads=(6,) * 6, window_size=16, num_tokens=128, reducted_dim=10,
                                                 mlp_ratio=2.0, upscale=4, upsampler='pixelshuffle'), (1, 3, 256, 256), torch.bfloat16, None, None),
        # RCAN x4 as published (10 groups x 20 RCABs, 64 features, reduction 16) and a light configuration (5 x 10)
        'rcan_x4_bf16_512': (synth.rcan_state_dict(scale=4, n_resgroups=10, n_resblocks=20, n_feats=64, reduction=16), (1, 3, 512, 512), torch.bfloat16, None, None),
        'rcan_light_x4_bf16_512': (synth.rcan_state_dict(scale=4, n_resgroups=5, n_resblocks=10, n_feats=64, reduction=16), (1, 3, 512, 512), torch.bfloat16, None, None),
        # GateR x1 restoration as published (dim 48, blocks 3-6-6-10-6-6-3), with the depthwise latent stage and with the focused linear attention
        'gater_bf16_512': (synth.gater_state_dict(dim=48, num_blocks=(3, 6, 6, 10, 6, 6, 3), latent_att=False), (1, 3, 512, 512), torch.bfloat16, None, None),
        'gater_att_bf16_512': (synth.gater_state_dict(dim=48, num_blocks=(3, 6, 6, 10, 6, 6, 3), latent_att=True), (1, 3, 512, 512), torch.bfloat16, None, None),
        # EIMN x2 at the reference's defaults (dim 64, 16 stages of one block, mlp ratio 2.66)
        'eimn_x2_512': (synth.eimn_state_dict(embed_dims=64, scale=2, num_stages=16), (1, 3, 512, 512), torch.bfloat16, None, None),
        # RHA x4 at the reference's defaults (dim 64, 4 groups x 6 blocks pooling by 8 / 4, window 8, pixelshuffledirect)
        'rha_x4_512': (synth.rha_state_dict(), (1, 3, 512, 512), torch.bfloat16, None, None),
        # FlexNet x4 at the reference's defaults (linear pipeline, dim 64, 6 LBlocks of 6 blocks, hidden_rate 4, ps head)
        'flexnet_x4_512': (synth.flexnet_state_dict(), (1, 3, 512, 512), torch.bfloat16, None, None),
        'compact_x4_fp16_b8_512': (synth.compact_state_dict(num_feat=64, num_conv=16, upscale=4), (8, 3, 512, 512), torch.float16, None, None),
        # Real-CUGAN: the 2x model at 1080p and the 4x model at 540p
        'cugan_x2_fp16_1080p': (synth.cugan_state_dict('2x'), (1, 3, 1080, 1920), torch.float16, None, None),
        'cugan_x4_fp16_540p': (synth.cugan_state_dict('4x'), (1, 3, 540, 960), torch.float16, None, None),
    }  # fmt: skip
    for name, (sd, shape, dt, flop_px, bytes_px) in cases.items():
        if args.only and args.only not in name:
            continue
        model = resselt_amd.load_from_state_dict(dict(sd)).to(dev)
        resolved = None
        for prec in ('auto', 'bf16x3'):
            model.precision = prec
            if prec != 'auto' and model.resolved_precision() == resolved:
                continue  # 'auto' already is this mode
            resolved = model.resolved_precision()
            x = synth.synth_input(shape, seed=0).to(dev).to(dt)
            y, t = timed(model, x, args.reps)
            out_px = y.shape[0] * y.shape[2] * y.shape[3]
            if hasattr(model, 'geometry'):  # per-pixel MACs that depend on the image size (Real-CUGAN's cropped U-Nets)
                macs = model.macs_per_input_pixel(shape[2], shape[3]) * shape[0] * shape[2] * shape[3]
            else:
                macs = (model.macs_per_input_pixel() if hasattr(model, 'macs_per_input_pixel') else 0) * shape[0] * shape[2] * shape[3]
            rec = dict(config=name, precision=prec if prec == resolved else f'{prec} -> {resolved}', in_shape=list(shape), io_dtype=str(dt).split('.')[-1], ms=round(t * 1e3, 3),
                       out_mp_s=round(out_px / 1e6 / t, 2), algorithmic_tflops=round(2 * macs / t / 1e12, 2),
                       launches=model.launches_per_forward(), finite=bool(torch.isfinite(y.float()).all()))  # fmt: skip
            if bytes_px:
                rec['layerwise_hbm_gbs'] = round(bytes_px * out_px / t / 1e9, 1)
            print(json.dumps(rec), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
