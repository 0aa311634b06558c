"""Shared helpers for the test-suite: golden fixture access and oracle dispatch."""

import glob
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    meta = json.loads(str(z['meta']))
    arrays = {k: torch.from_numpy(z[k]) for k in z.files if k != 'meta'}
    return meta, arrays


def golden_names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + '*.npz')))


def synth_state_dict(meta):
    from resselt_amd.utils import synth

    kw = dict(meta['synth'])
    for k in ('blocks', 'depth', 'depths', 'num_heads', 'split_size', 'scale_list'):
        if k in kw:
            kw[k] = tuple(kw[k])
    fn = {'esrgan': synth.rrdbnet_state_dict, 'spanplus': synth.spanplus_state_dict, 'span': synth.span_state_dict,
          'swinir': getattr(synth, 'swinir_state_dict', None), 'compact': synth.compact_state_dict, 'dat': getattr(synth, 'dat_state_dict', None), 'spanpp': getattr(synth, 'spanpp_state_dict', None), 'hat': getattr(synth, 'hat_state_dict', None), 'rtmosr': getattr(synth, 'rtmosr_state_dict', None), 'drct': getattr(synth, 'drct_state_dict', None), 'plksr': synth.plksr_state_dict, 'realplksr': synth.realplksr_state_dict, 'cugan': synth.cugan_state_dict}[meta['arch']]  # fmt: skip
    return fn(seed=meta['seed'], **kw)


def oracle_forward(meta, sd, x):
    if meta['arch'] == 'esrgan':
        from oracle.rrdbnet import rrdbnet_forward

        return rrdbnet_forward(sd, x)
    if meta['arch'] == 'spanplus':
        from oracle.span import spanplus_forward

        return spanplus_forward(sd, x)
    if meta['arch'] == 'span':
        from oracle.span import span_forward

        return span_forward(sd, x)
    if meta['arch'] == 'swinir':
        from oracle.swinir import swinir_forward

        return swinir_forward(sd, x)
    if meta['arch'] == 'compact':
        from oracle.compact import compact_forward

        return compact_forward(sd, x)
    if meta['arch'] == 'spanpp':
        from oracle.spanpp import spanpp_forward

        return spanpp_forward(sd, x, meta.get('scale'))
    if meta['arch'] == 'rtmosr':
        from oracle.rtmosr import rtmosr_forward

        return rtmosr_forward(sd, x)
    if meta['arch'] == 'hat':
        from oracle.hat import hat_forward

        return hat_forward(sd, x)
    if meta['arch'] == 'drct':
        from oracle.drct import drct_forward

        return drct_forward(sd, x)
    if meta['arch'] == 'dat':
        from oracle.dat import dat_forward

        return dat_forward(sd, x)
    if meta['arch'] in ('plksr', 'realplksr'):
        from oracle.plksr import plksr_forward

        return plksr_forward(sd, x)
    if meta['arch'] == 'cugan':
        from oracle.cugan import cugan_forward

        return cugan_forward(sd, x)
    # The families whose oracles live next to the tests (tests/<arch>_oracle.py).  They compute in the dtype of ``x``; what the forward needs
    # beyond the state dict travels in ``meta``.
    if meta['arch'] == 'mosr':
        from mosr_oracle import mosr_forward

        return mosr_forward(sd, x, meta.get('upsampler', 'ps'), meta['upscale'])
    if meta['arch'] == 'mosrv2':
        from mosr_oracle import mosrv2_forward

        return mosrv2_forward(sd, x, meta.get('upsampler', 'pixelshuffledirect'), meta['upscale'], meta.get('mid_dim', 32))
    if meta['arch'] == 'rgt':
        from rgt_oracle import rgt_forward

        return rgt_forward(sd, x, tuple(meta['split_size']), tuple(meta['num_heads']), meta.get('c_ratio', 0.5))
    if meta['arch'] == 'atd':
        from atd_oracle import atd_forward

        return atd_forward(sd, x, meta['hyper'], force=meta.get('force'), record=meta.get('record'))
    if meta['arch'] in ('fdat', 'omnisr', 'rcan', 'gater', 'eimn', 'rha', 'flexnet', 'moesr', 'smosr', 'gfisrv2'):
        import importlib

        return getattr(importlib.import_module(f'{meta["arch"]}_oracle'), f'{meta["arch"]}_forward')(sd, x)
    raise KeyError(meta['arch'])
