"""``fold_doconv`` / ``fold_convnxc`` (resselt_amd/archs/smosr/arch.py) against the unfolded train-mode chains in float64: the folded
weight and bias, applied as ONE zero-padded convolution, reproduce DOConv2d's ``conv2d(x, DoW * mul, bias * mul)`` and ConvNXC's
1x1 -> k x k -> 1x1 on the zero-padded input plus ``sk`` to 1e-12 relative, for 3x3 and 1x1 kernels and ``mul`` != 1; and no ``eval_conv``
tensor takes part."""

import pytest
import torch
import torch.nn.functional as F

import smosr_oracle as O
from resselt_amd.archs.smosr.arch import SMoSR, _conv_shapes, fold, fold_convnxc, fold_doconv
from resselt_amd.utils import synth

REL = 1e-12


def _module_sd(ci, co, k, rep, seed, mul=1.0):
    """A synthetic DOConv2d / ConvNXC under the prefix 'm', float64, drawn as synth.smosr_state_dict draws them (mul far from 1)."""
    shapes, muls = {}, {}
    _conv_shapes(shapes, muls, 'm', ci, co, k, rep, mul=mul)
    sd = {}
    for key, shape in shapes.items():
        leaf = key.rsplit('.', 1)[1]
        if '.eval_conv.' in key:
            sd[key] = synth.synth_tensor(key, shape, 1, seed)
        elif leaf == 'mul':
            sd[key] = muls[key] * (1.0 + synth.synth_tensor(key, shape, 1, seed, 0.3))
        elif leaf == 'W':
            sd[key] = synth.synth_tensor(key, shape, shape[1] * shape[2], seed, 1.5)
        elif leaf == 'D':
            sd[key] = synth.synth_tensor(key, shape, 1, seed, 0.2)
        elif leaf == 'd_diag':
            sd[key] = torch.eye(shape[1]).reshape(1, shape[1], shape[1]).repeat(shape[0], 1, 1)
        else:
            sd[key] = synth.synth_tensor(key, shape, 4, seed)
    return {k: v.double() for k, v in sd.items()}


@pytest.mark.parametrize('rep', [False, True], ids=['doconv', 'convnxc'])
@pytest.mark.parametrize('ci,co,k,mul', [(5, 7, 3, 3.0), (6, 4, 1, 0.02), (3, 16, 3, 1.0), (8, 8, 1, 3.0)])
def test_fold_reproduces_the_unfolded_chain(rep, ci, co, k, mul):
    sd = _module_sd(ci, co, k, rep, seed=7 + ci, mul=mul)
    assert all(abs(float(v) - 1.0) > 1e-3 for key, v in sd.items() if key.endswith('.mul'))
    x = synth.synth_input((2, ci, 6, 7), 3).double() - 0.5
    want = O.conv(sd, 'm', x)  # the chain as trained: smosr_oracle evaluates it unfolded
    w, b = fold(sd, 'm', rep)
    assert w.dtype == torch.float64 and tuple(w.shape) == (co, ci, k, k) and tuple(b.shape) == (co,)
    got = F.conv2d(x, w, b, padding=k // 2)
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f'MEASURE fold rep={rep} {ci}->{co} k{k} mul {mul}: relative {err:.2e}')
    assert err <= REL
    assert (fold_convnxc if rep else fold_doconv)(sd, 'm')[0].equal(w)


def test_doconv_1x1_is_w_times_mul():
    sd = _module_sd(6, 4, 1, False, seed=2, mul=0.5)
    w, b = fold_doconv(sd, 'm')
    assert 'm.D' not in sd and torch.equal(w[:, :, 0, 0], sd['m.W'][:, :, 0] * sd['m.mul']) and torch.equal(b, sd['m.bias'] * sd['m.mul'])


@pytest.mark.parametrize('rep', [False, True])
def test_eval_conv_tensors_change_nothing(rep):
    kw = dict(dim=16, n_mb=1, rep=rep, upsampler='pa_up', upsampler_mid_dim=8, seed=4)
    sd = synth.smosr_state_dict(**kw)
    m = SMoSR(**{k: v for k, v in kw.items() if k != 'seed'})
    m.load_state_dict(sd)
    a = m.folded_state()
    other = {k: (torch.full_like(v, 123.0) if '.eval_conv.' in k else v) for k, v in sd.items()}
    assert sum('.eval_conv.' in k for k in sd) > 20
    m.load_state_dict(other)
    b = m.folded_state()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not any('eval_conv' in k or k.endswith(('.W', '.D', '.mul', '.d_diag')) for k in a)
    x = synth.synth_input((1, 3, 5, 6), 1)
    assert torch.equal(O.smosr_forward(sd, x), O.smosr_forward(other, x))
