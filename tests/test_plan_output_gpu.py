"""Every forward returns a fresh output tensor, and reads the input it was given: two consecutive forwards with different inputs, one
fixture per architecture (the heads that add the input back as a base image among them)."""

import pytest
import torch

import resselt_amd
from helpers import load_golden, synth_state_dict

pytestmark = pytest.mark.gpu

FIXTURES = [
    'compact_x2_nf32_nc4_b2_17x19',
    'cugan_x4_21x25',  # nearest x4 of the input added in the output stage
    'dat_x2_e64_s2x4_d3_1_3conv_direct_13x18',
    'drct_x2_e60_g16_w8_identity_b2_24x40',  # one output slice per image
    'hat_x2_e60_w8_d2_2_20x27',
    'plksr_x2_ccm_d32_b2_15x17',
    'realplksr_x2_dys_d64_b2_20x24',
    'rrdbnet_x2plus_unshuffle_nb2_21x30',
    'rtmosr_x2_d32_b2_13x17',
    'span_x2_nonorm_19x21',
    'spanplus_dys_x2_24x40',
    'spanpp_fc48_x2_default_24x40',
    'swinir_dn_gray_19x21',  # the denoising head adds the caller's input back
]


@pytest.fixture(autouse=True)
def _no_failed_hand_offs():
    yield
    from resselt_amd.engine import lib as L

    if torch.cuda.is_available():
        torch.cuda.synchronize()
        L.check_status('end of test')


def _two_forwards(m, x1, x2):
    ya = m(x1)
    ya_copy = ya.clone()
    yb = m(x2)
    yc = m(x1.clone())  # the first input again, at another address
    torch.cuda.synchronize()
    assert ya.data_ptr() != yb.data_ptr() and yb.data_ptr() != yc.data_ptr()
    assert torch.equal(ya, ya_copy)  # the second forward left the first result alone
    assert not torch.equal(ya, yb)
    assert torch.equal(yc, ya)


@pytest.mark.parametrize('name', FIXTURES)
def test_consecutive_forwards_return_fresh_outputs(device, name):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(synth_state_dict(meta))).to(device)
    x1 = arr['x'].to(device)
    _two_forwards(m, x1, x1.flip(-1).contiguous())


@pytest.mark.parametrize('name', ['rrdbnet_x2_nb3_b2_19x27', 'cugan_x2_23x22'])
def test_consecutive_u8_forwards_return_fresh_outputs(device, name):
    meta, arr = load_golden(name)
    m = resselt_amd.load_from_state_dict(dict(synth_state_dict(meta))).to(device)
    img = (arr['x'].clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(device)
    _two_forwards(m, img, img.flip(2).contiguous())


@pytest.mark.parametrize('mode', ['banded', 'graph'])
def test_consecutive_rrdbnet_forwards_return_fresh_outputs(device, mode):
    meta, arr = load_golden('rrdbnet_x2_nb3_b2_19x27')
    m = resselt_amd.load_from_state_dict(dict(synth_state_dict(meta))).to(device)
    if mode == 'banded':
        m.tail_band_rows = 16  # two bands of the 19 rows (before the first plan is built): the band copies write the plan's current output
    else:
        m.use_graph = True
    x1 = arr['x'].to(device)
    _two_forwards(m, x1, x1.flip(-1).contiguous())
