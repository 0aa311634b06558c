#!/usr/bin/env python3
"""(Lives under tests/: like the test-suite it uses the CPU oracle as the checker.)

Randomised parity sweep on the GPU: every architecture x odd sizes x batch x tensor dtype against the CPU oracle.

usage: python tests/fuzz_parity.py [seed] [cases_per_arch]   -> one line per case, non-zero exit status on the first failure
"""

import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

import resselt_amd  # noqa: E402
from helpers import oracle_forward  # noqa: E402
from resselt_amd.utils import synth  # noqa: E402


def _cugan_accepts(sd, h, w):
    from oracle.cugan import cugan_variant
    from resselt_amd.archs.cugan.arch import cugan_layers

    try:
        cugan_layers(cugan_variant(sd), 3, 3, h, w)
    except ValueError:
        return False
    return True


def _oracle_accepts(meta, sd, h, w):
    """The oracles of tests/<arch>_oracle.py raise exactly where the reference does (the plans refuse those sizes too)."""
    try:
        with torch.no_grad():
            oracle_forward(meta, sd, synth.synth_input((1, 3, h, w), seed=0))
    except Exception:
        return False
    return True


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    per_arch = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    rng = random.Random(seed)
    dev = torch.device('cuda:0')
    makers = {
        'esrgan': lambda s: (synth.rrdbnet_state_dict(nb=rng.choice([1, 2, 3]), scale=rng.choice([1, 2, 4]), plus=rng.random() < 0.3, seed=s), 1),
        'spanplus': lambda s: (synth.spanplus_state_dict(upscale=rng.choice([2, 3, 4]), upsampler=rng.choice(['ps', 'dys']), seed=s), 1),
        'span': lambda s: (synth.span_state_dict(upscale=rng.choice([2, 4]), seed=s), 1),
        'spanpp': lambda s: (synth.spanpp_state_dict(feature_channels=32, implicit_dim=32, latent_layers=2, seed=s), 1),
        'compact': lambda s: (synth.compact_state_dict(num_feat=rng.choice([32, 64]), num_conv=rng.choice([2, 5]), upscale=rng.choice([2, 4]), seed=s), 1),
        'swinir': lambda s: (synth.swinir_state_dict(embed_dim=60, depths=(2, 2), num_heads=(6, 6), upscale=rng.choice([2, 4]),
                                                     upsampler=rng.choice(['nearest+conv', 'pixelshuffle', 'pixelshuffledirect']), seed=s), 9),
        'swinir_restore': lambda s: ((lambda w7: synth.swinir_state_dict(in_ch=rng.choice([1, 3]), embed_dim=60, depths=(2, 2), num_heads=(6, 6), upscale=1,
                                                                         upsampler='', window=7 if w7 else 8, img_size=126 if w7 else 64, seed=s))(rng.random() < 0.5), 9),
        'dat': lambda s: (synth.dat_state_dict(embed_dim=64, depth=(3,), num_heads=(4,), split_size=rng.choice([(2, 4), (4, 8), (8, 8)]),
                                               upscale=rng.choice([2, 3]), img_size=16, seed=s), 2),
        'rtmosr': lambda s: (synth.rtmosr_state_dict(scale=rng.choice([2, 4]), dim=rng.choice([32, 48]), n_blocks=2, se=rng.random() < 0.6,
                                                     dccm=rng.random() < 0.7, seed=s), 3),
        'drct': lambda s: (synth.drct_state_dict(embed_dim=rng.choice([60, 96]), gc=16, window=rng.choice([4, 8]), num_layers=rng.choice([1, 2]), upscale=rng.choice([2, 3, 4]),
                                                 mlp_ratio=rng.choice([2.0, 4.0]), seed=s), 9),
        'esrganbig': lambda s: (synth.rrdbnet_state_dict(nb=2, scale=4, seed=s), 1),
        'hat': lambda s: (synth.hat_state_dict(embed_dim=60, depths=(2,), num_heads=(6,), window=rng.choice([4, 8]), upscale=rng.choice([2, 4]), seed=s), 9),
        'plksr': lambda s: ((lambda lk: synth.plksr_state_dict(dim=32, n_blocks=rng.choice([1, 2]), upscale=rng.choice([1, 2, 3, 4]), ccm_type=rng.choice(['CCM', 'ICCM', 'DCCM']),
                                                               kernel_size=17 if lk == 'SparsePLK' else rng.choice([9, 17, 27]), lk_type=lk, use_ea=rng.random() < 0.7,
                                                               seed=s))(rng.choice(['PLK', 'SparsePLK', 'RectSparsePLK'])), 1),
        'realplksr': lambda s: (synth.realplksr_state_dict(dim=rng.choice([32, 64]), n_blocks=2, upscale=rng.choice([1, 2, 3, 4]), kernel_size=rng.choice([9, 17, 31]),
                                                           use_ea=rng.random() < 0.7, dysample=rng.random() < 0.5, seed=s), 1),
        'cugan': lambda s: ((lambda v: synth.cugan_state_dict(v, pro=v != '2x_fast' and rng.random() < 0.5, seed=s))(rng.choice(['2x', '3x', '4x', '2x_fast'])), 16),
        # the families whose oracles are tests/<arch>_oracle.py: a third element carries what the oracle needs besides the state dict
        # (helpers.oracle_forward); sizes their oracle refuses are redrawn.  ATD is not here: its category sort makes a free-running
        # comparison ill-defined (tests/atd_trajectory.py).
        'mosr': lambda s: ((lambda up, sc: (synth.mosr_state_dict(upscale=sc, n_block=rng.choice([1, 2]), dim=rng.choice([32, 48]), upsampler=up,
                                                                  kernel_size=rng.choice([3, 5, 7]), seed=s), 1, dict(upsampler=up, upscale=sc)))
                           (rng.choice(['ps', 'dys', 'gps']), rng.choice([2, 3, 4]))),
        'mosrv2': lambda s: ((lambda up, sc, un: (synth.mosrv2_state_dict(scale=sc, n_block=rng.choice([1, 2]), dim=32, upsampler=up, unshuffle_mod=un,
                                                                          rms_norm=rng.random() < 0.5, seed=s), 2, dict(upsampler=up, upscale=sc)))
                             (rng.choice(['pixelshuffledirect', 'pixelshuffle', 'nearest+conv']), rng.choice([1, 2, 4]), rng.random() < 0.6)),
        'rgt': lambda s: ((lambda sp, nh: (synth.rgt_state_dict(embed_dim=32, depth=(2,), num_heads=(nh,), split_size=sp, upscale=rng.choice([2, 3, 4]), seed=s), 16,
                                           dict(split_size=sp, num_heads=(nh,))))(rng.choice([(2, 4), (4, 8), (4, 4)]), rng.choice([2, 4]))),
        'fdat': lambda s: (synth.fdat_state_dict(scale=rng.choice([2, 4]), embed_dim=rng.choice([32, 48]), num_groups=1, depth_per_group=2, num_heads=4, window_size=rng.choice([4, 8]),
                                                 upsampler_type=rng.choice(['pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'transpose+conv', 'lda', 'pa_up']),
                                                 unshuffle_mod=rng.random() < 0.3, seed=s), 1),
        'omnisr': lambda s: (synth.omnisr_state_dict(num_feat=32, window_size=rng.choice([4, 8]), up_scale=rng.choice([2, 3, 4]), pe=rng.random() < 0.7, seed=s), 9),
        'rcan': lambda s: (synth.rcan_state_dict(scale=rng.choice([2, 4]), n_resgroups=rng.choice([1, 2]), n_resblocks=2, n_feats=rng.choice([32, 48, 64]), norm=rng.random() < 0.5,
                                                 unshuffle_mod=rng.random() < 0.4, seed=s), 1),
        'gater': lambda s: (synth.gater_state_dict(dim=24, num_blocks=(1,) * 7, latent_att=rng.random() < 0.6, seed=s), 5),
        'eimn': lambda s: (synth.eimn_state_dict(embed_dims=rng.choice([32, 64]), scale=rng.choice([2, 3, 4]), num_stages=rng.choice([1, 2]), seed=s), 1),
        'rha': lambda s: ((lambda dl: synth.rha_state_dict(dim=32, scale=rng.choice([2, 3, 4]), down_list=dl, window_size=rng.choice([4, 8]), group_blocks=1, res_blocks=2,
                                                           upsample=rng.choice(['pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample']), seed=s))
                          (rng.choice([(2, 1), (1,), (2,), (4, 2)])), 5),
        'flexnet': lambda s: (synth.flexnet_state_dict(seed=s, dim=rng.choice([32, 48]), num_blocks=rng.choice([(1, 1), (2,), (1, 2)]), scale=rng.choice([2, 3, 4]),
                                                       upsampler=rng.choice(['ps', 'dys', 'n+c']), channel_norm=rng.random() < 0.3), 5),
        'moesr': lambda s: (synth.moesr_state_dict(scale=rng.choice([2, 3, 4]), dim=rng.choice([32, 48]), n_blocks=rng.choice([1, 2]), n_block=rng.choice([1, 2]),
                                                   upsampler=rng.choice(['pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample']), seed=s), 2),
        'smosr': lambda s: ((lambda up: synth.smosr_state_dict(dim=rng.choice([32, 48]), scale=rng.choice([2, 3, 4] if up != 'nearest+conv' else [2, 4]),
                                                               rep=up != 'dysample' and rng.random() < 0.4, n_mb=rng.choice([1, 2]), upsampler=up,
                                                               d_kernel=rng.choice([1, 3]), seed=s))
                            (rng.choice(['pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample', 'pa_up'])), 3),
        'gfisrv2': lambda s: (synth.gfisrv2_state_dict(dim=rng.choice([16, 32]), scale=rng.choice([2, 3, 4]), n_blocks=rng.choice([1, 2]),
                                                       upsampler=rng.choice(['pixelshuffledirect', 'pixelshuffle', 'nearest+conv', 'dysample']), seed=s), 2),
    }  # fmt: skip
    own_oracle = ('mosr', 'mosrv2', 'rgt', 'fdat', 'omnisr', 'rcan', 'gater', 'eimn', 'rha', 'flexnet', 'moesr', 'smosr', 'gfisrv2')
    worst = 0.0
    for arch, make in makers.items():
        for k in range(per_arch):
            s = rng.randrange(1 << 20)
            sd, min_hw, *extra = make(s)
            meta = dict(extra[0] if extra else {}, arch='esrgan' if arch == 'esrganbig' else arch.split('_')[0])
            n = 1 if arch == 'drct' else rng.choice([1, 1, 2, 3])
            h, w = rng.randint(min_hw, 45), rng.randint(min_hw, 45)
            if arch == 'esrganbig':  # many tiles per workgroup, ragged edges, a row-banded tail
                h, w = rng.randint(300, 420), rng.randint(500, 700)
            while arch == 'cugan' and not _cugan_accepts(sd, h, w):  # the sizes the reference refuses (the plan refuses them too)
                h, w = rng.randint(min_hw, 90), rng.randint(min_hw, 90)
            while arch in own_oracle and not _oracle_accepts(meta, sd, h, w):  # likewise: a reflect pad wider than the image, RG-SA below 16, ...
                h, w = rng.randint(min_hw, 45), rng.randint(min_hw, 45)
            dt = rng.choice([torch.float32, torch.float32, torch.float16, torch.bfloat16])
            cin = sd['conv_first.weight'].shape[1] if arch == 'swinir_restore' else 3
            x = synth.synth_input((n, cin, h, w), seed=s).to(dt)
            with torch.no_grad():
                ref = oracle_forward(meta, sd, x.float())
            model = resselt_amd.load_from_state_dict(dict(sd)).to(dev)
            if arch == 'esrganbig':
                model.tail_band_rows = rng.choice([64, 100, 4096])
            xd = x.to(dev)
            if rng.random() < 0.3:  # a non-contiguous view of the same values
                xd = xd.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
            y = model(xd)
            torch.cuda.synchronize()
            scale = max(1.0, ref.abs().max().item())
            tol = {torch.float32: 3e-4, torch.float16: 2e-3, torch.bfloat16: 1.2e-2}[dt] * scale
            err = (y.float().cpu() - ref).abs().max().item()
            ok = y.shape == ref.shape and y.dtype == dt and err <= tol
            worst = max(worst, err / tol)
            print(f'{arch:14s} n={n} {h:2d}x{w:2d} {str(dt).split(".")[-1]:8s} -> {tuple(y.shape)} max-abs {err:.2e} (tol {tol:.1e}) {"ok" if ok else "FAIL"}', flush=True)
            if not ok:
                raise SystemExit(1)
            del model
    print(f'all cases passed; worst error / tolerance = {worst:.3f}')


if __name__ == '__main__':
    main()
