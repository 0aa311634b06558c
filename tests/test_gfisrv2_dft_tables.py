"""The host-side DFT tables of rsa_gfisr_dft (resselt_amd/engine/lib_gfisr.py) against ``torch.fft`` in float64: rfft2 and irfft2 with
norm='ortho', the inverse on NON-Hermitian half spectra (non-zero imaginary parts in column 0 and in the Nyquist column, which irfft2
ignores).  Bar 1e-12.  Also the layouts the header gives and the single rounding to f32."""

import numpy as np
import pytest
import torch

from resselt_amd.engine import lib_gfisr as LG

SIZES = [(5, 7), (6, 8), (2, 1), (1, 2), (13, 16), (17, 9)]
BAR = 1e-12


@pytest.mark.parametrize('H,W', SIZES)
def test_forward_and_inverse_match_torch_fft(H, W):
    gen = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn(2, 3, H, W, dtype=torch.float64, generator=gen) + 2.0
    z = LG.rfft2_f64(x)
    ref = torch.fft.rfft2(x, norm='ortho')
    fwd = max((z[..., 0, :, :] - ref.real).abs().max().item(), (z[..., 1, :, :] - ref.imag).abs().max().item())
    s = torch.randn(2, 3, 2, H, W // 2 + 1, dtype=torch.float64, generator=gen)  # not Hermitian
    assert s[..., 1, :, 0].abs().min() > 0
    y = LG.irfft2_f64(s, H, W)
    inv = (y - torch.fft.irfft2(torch.complex(s[..., 0, :, :], s[..., 1, :, :]), s=(H, W), norm='ortho')).abs().max().item()
    print(f'MEASURE {H}x{W}: forward {fwd:.2e}, inverse {inv:.2e} (bar {BAR:.0e})')
    assert fwd <= BAR and inv <= BAR


@pytest.mark.parametrize('H,W', [(6, 8), (5, 7), (1, 2)])
def test_the_imaginary_parts_of_column_0_and_nyquist_do_not_contribute(H, W):
    t = LG.dft_tables_f64(H, W)
    Wf = W // 2 + 1
    assert np.abs(t['row_inv'][Wf]).max() == 0.0  # -c_0 sin(0)
    if W % 2 == 0:
        assert np.abs(t['row_inv'][Wf + W // 2]).max() < 1e-15  # sin(pi x): zero but for the rounding of pi
        assert np.allclose(np.abs(t['row_inv'][W // 2]), 1 / np.sqrt(W))  # c = 1 there
    assert np.allclose(t['row_inv'][0], 1 / np.sqrt(W))


def test_layouts_and_rounding():
    H, W = 5, 8
    Wf = W // 2 + 1
    t64 = LG.dft_tables_f64(H, W)
    assert t64['row_fwd'].shape == (W, 2 * Wf) and t64['row_inv'].shape == (2 * Wf, W)
    assert t64['col_fwd'].shape == t64['col_inv'].shape == (2 * H, 2 * H)
    assert np.array_equal(t64['col_fwd'], t64['col_inv'].T)  # the inverse column transform is the transpose of the forward one
    # the index product is reduced before the angle is taken: entries a whole period apart are bit-equal
    assert LG._angles(np.array([4095]), np.array([4095]), 4096)[0, 0] == LG._angles(np.array([1]), np.array([1]), 4096)[0, 0]
    t32 = LG.dft_tables(H, W, 'cpu')
    for k, v in t64.items():
        assert t32[k].dtype == torch.float32 and t32[k].is_contiguous() and np.array_equal(t32[k].numpy(), v.astype(np.float32))
