"""Pins of ``macs_per_input_pixel()`` and of the parameter tree (the sorted ``(key, shape)`` list of ``state_dict()``) of the transformer
models, one configuration per head and tail kind.  The expected values were recorded at the commit BEFORE the residual tails and the
reconstruction heads moved to engine/transformer.py: a shared helper that changes a count or a key moves one of these."""

import hashlib
import importlib

import pytest

# (model, constructor arguments, MACs per input pixel, state_dict keys, sha256 of repr(sorted (key, shape) list)[:16])
PINS = [
    ('SwinIR', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'upscale': 4, 'upsampler': 'pixelshuffle', 'resi_connection': '1conv'}, 1044228, 78, '7e7d6a50ebe34140'),
    ('SwinIR', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'upscale': 3, 'upsampler': 'pixelshuffle', 'resi_connection': '3conv'}, 578703, 88, '3aaed34f026ffd72'),
    ('SwinIR', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'upscale': 4, 'upsampler': 'nearest+conv', 'resi_connection': '3conv'}, 1586127, 92, 'c2f818239dd65ec9'),
    ('SwinIR', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'upscale': 2, 'upsampler': 'nearest+conv', 'resi_connection': '1conv'}, 581124, 78, '0ec01ee097601dc9'),
    ('SwinIR', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'upscale': 2, 'upsampler': 'pixelshuffledirect', 'resi_connection': '1conv'}, 251220, 72, '8e42d9016758f391'),
    ('SwinIR', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'upscale': 1, 'upsampler': '', 'resi_connection': '3conv'}, 198435, 84, 'a8922c0f40716c2a'),
    ('DAT', {'embed_dim': 48, 'split_size': (8, 16), 'depth': (2, 2), 'num_heads': (4, 4), 'expansion_factor': 2.0, 'upscale': 4, 'upsampler': 'pixelshuffle', 'resi_connection': '1conv'}, 950928, 252, 'ed5360129f6602d5'),
    ('DAT', {'embed_dim': 48, 'split_size': (8, 16), 'depth': (2, 2), 'num_heads': (4, 4), 'expansion_factor': 2.0, 'upscale': 3, 'upsampler': 'pixelshuffle', 'resi_connection': '3conv'}, 502656, 262, 'baa0ad87ccbfd897'),
    ('DAT', {'embed_dim': 48, 'split_size': (8, 16), 'depth': (2, 2), 'num_heads': (4, 4), 'expansion_factor': 2.0, 'upscale': 2, 'upsampler': 'pixelshuffledirect', 'resi_connection': '3conv'}, 132864, 258, '337e59b3cc8eaabf'),
    ('RGT', {'embed_dim': 48, 'depth': (2, 2), 'num_heads': (4, 4), 'mlp_ratio': 2.0, 'split_size': (8, 8), 'upscale': 2, 'resi_connection': '1conv'}, 454738, 184, 'd39bbfbbd3fd172f'),
    ('RGT', {'embed_dim': 48, 'depth': (2, 2), 'num_heads': (4, 4), 'mlp_ratio': 2.0, 'split_size': (8, 8), 'upscale': 3, 'resi_connection': '3conv'}, 617026, 196, 'bb6e59e4921b4dc7'),
    ('ATD', {'embed_dim': 48, 'depths': (2, 2), 'num_heads': (4, 4), 'upscale': 4, 'upsampler': 'pixelshuffle', 'resi_connection': '1conv'}, 1091728, 129, 'cb8ee16e94094978'),
    ('ATD', {'embed_dim': 48, 'depths': (2, 2), 'num_heads': (4, 4), 'upscale': 3, 'upsampler': 'pixelshuffle', 'resi_connection': '3conv'}, 643456, 139, '1a025cc3ab726eed'),
    ('ATD', {'embed_dim': 48, 'depths': (2, 2), 'num_heads': (4, 4), 'upscale': 4, 'upsampler': 'nearest+conv', 'resi_connection': '3conv'}, 1650880, 143, 'ab1775c935279c8a'),
    ('ATD', {'embed_dim': 48, 'depths': (2, 2), 'num_heads': (4, 4), 'upscale': 2, 'upsampler': 'pixelshuffledirect', 'resi_connection': '1conv'}, 304336, 123, '5bca5b498b3c61cd'),
    ('ATD', {'embed_dim': 48, 'depths': (2, 2), 'num_heads': (4, 4), 'upscale': 1, 'upsampler': '', 'resi_connection': '3conv'}, 269776, 135, '0cf6f9b21ae734e5'),
    ('HAT', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'upscale': 4, 'resi_connection': '1conv'}, 1222788, 132, 'c766e640c4b1a885'),
    ('HAT', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'upscale': 3, 'resi_connection': 'identity', 'num_feat': 32}, 434100, 124, 'e1dfc553d4fd7741'),
    ('DRCT', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'gc': 16, 'upsampler': 'pixelshuffle', 'upscale': 4, 'resi_connection': '1conv'}, 1586820, 180, 'c33dc2baea6628c5'),
    ('DRCT', {'embed_dim': 60, 'depths': (2, 2), 'num_heads': (6, 6), 'window_size': 8, 'mlp_ratio': 2.0, 'gc': 16, 'upsampler': 'pixelshuffle', 'upscale': 3, 'resi_connection': 'identity'}, 1136820, 176, 'a10e0e16ce000403'),
]


@pytest.mark.parametrize('name,kwargs,macs,nkeys,digest', PINS, ids=[f"{p[0]}-x{p[1]['upscale']}-{p[1].get('upsampler', 'pixelshuffle') or 'none'}-{p[1]['resi_connection']}" for p in PINS])
def test_macs_and_parameter_tree_are_pinned(name, kwargs, macs, nkeys, digest):
    model = getattr(importlib.import_module(f'resselt_amd.archs.{name.lower()}.arch'), name)(**kwargs)
    items = sorted((k, tuple(v.shape)) for k, v in model.state_dict().items())
    print(name, kwargs, model.macs_per_input_pixel(), len(items))
    assert model.macs_per_input_pixel() == macs
    assert len(items) == nkeys
    assert hashlib.sha256(repr(items).encode()).hexdigest()[:16] == digest
