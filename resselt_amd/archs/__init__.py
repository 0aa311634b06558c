"""Architectures served by the MI355X engine, registered explicitly in detection order.

The reference discovers 31 architectures by walking the filesystem (``resselt/archs/__init__.py:11-28``);
this build registers the families of the hot path: ESRGAN/RRDBNet, SPANPlus, SPAN, SwinIR, DAT, HAT, and the "next" rows of §8f built so far (Compact, SpanPP, RTMoSR, MoSR, MoSRv2, PLKSR / RealPLKSR, Real-CUGAN, RGT, FDAT, OmniSR, ATD, RCAN, GateR, EIMN, RHA, FlexNet, MoESR, SMoSR, GFISRv2, FIGSR, LAWFFT, GFISR, GateRV3, GateRv2); the first
"next" row of §8f (Compact / SRVGGNetCompact, pure reuse of the conv kernel).
"""

from ..registry import Registry
from .atd import ATDArch
from .compact import CompactArch
from .cugan import CUGANArch
from .dat import DatArch
from .drct import DRCTArch
from .eimn import EIMNArch
from .esrgan import ESRGANArch
from .fdat import FDATArch
from .figsr import FIGSRArch
from .flexnet import FlexNetArch
from .gater import GateRArch
from .gaterv2 import GateRV2Arch
from .gaterv3 import GateRV3Arch
from .gfisr import GFISRArch
from .gfisrv2 import GFISRV2Arch
from .hat import HATArch
from .lawfft import LAWFFTArch
from .moesr import MoESRArch
from .mosr import MoSRArch
from .mosrv2 import MoSRv2Arch
from .omnisr import OmniSRArch
from .plksr import PLKSRArch
from .rcan import RCANArch
from .rgt import RGTArch
from .rha import RHAArch
from .rtmosr import RTMoSRArch
from .smosr import SMoSRArch
from .span import SPANArch
from .spanplus import SpanPlusArch
from .spanpp import SpanPPArch
from .swinir import SwinIRArch

internal_registry = Registry()
# relative order follows the reference's registry walk (tests/golden/registry_claims.npz): eimn, ESRGAN, HAT, dat, RCAN, Compact, GateR, ATD, RGT, OmniSR, MoSR, FDAT, CuGAN, PLKSR, MoSRv2, RTMoSR,
# spanplus, SwinIR, SpanPP, ..., SPAN
for _arch in (EIMNArch, ESRGANArch, HATArch, DatArch, RCANArch, CompactArch, GateRArch, ATDArch, RGTArch, OmniSRArch, MoSRArch, FDATArch, CUGANArch, PLKSRArch, MoSRv2Arch, RTMoSRArch, SpanPlusArch, SwinIRArch, SpanPPArch, DRCTArch, SPANArch):
    internal_registry.add(_arch())
# RHA is consulted after the walk (``Registry.late``): no other architecture matches its keys and it matches nobody else's checkpoints
# (tests/test_rha_loader.py checks both against every registered architecture), so where it stands cannot change who loads what.  The
# reference walks it between dat and RCAN.
internal_registry.add(RHAArch(), late=True)
# FlexNet likewise (tests/test_flexnet_loader.py checks the same two properties), one tier further back (``Registry.last``): the contents
# of ``late`` and what iterating over the registry yields stay what they were.  The reference walks it between ESRGAN and HAT.
internal_registry.add(FlexNetArch(), last=True)
# MoESR likewise (tests/test_moesr_loader.py), in ``Registry.after``: the open-ended tier consulted once ``walk()`` has declined, so that
# ``late``, ``last``, ``walk()`` and what iterating over the registry yields stay what they were.  The reference walks it right behind RTMoSR.
internal_registry.add(MoESRArch(), after=True)
# SMoSR likewise (tests/test_smosr_loader.py), in ``Registry.tail``, consulted once ``consulted()`` has declined: ``after`` and
# ``consulted()`` are held to ``walk()`` + MoESR by tests/test_moesr_loader.py, so they stay what they were too.  The reference walks it
# between PLKSR and MoSRv2.
internal_registry.add(SMoSRArch(), tail=True)
# GFISRv2 likewise (tests/test_gfisrv2_loader.py), in ``Registry.rest``: the open-ended tier consulted once ``every()`` has declined, which
# tests/test_smosr_loader.py holds to ``consulted()`` + SMoSR.  Later architectures of this kind go into ``rest`` too.
internal_registry.add(GFISRV2Arch(), rest=True)
# FIGSR, the next of the GFISR family (tests/test_figsr_loader.py checks the same two properties), goes into ``rest`` behind GFISRv2: every
# older tier and iterator stays what it was.
internal_registry.add(FIGSRArch(), rest=True)
# LAWFFT likewise (tests/test_lawfft_loader.py checks the same two properties), in ``rest`` behind FIGSR: tests/test_figsr_loader.py holds
# ``rest[:2]``.
internal_registry.add(LAWFFTArch(), rest=True)
# GFISR (v1), the model those three descend from (tests/test_gfisr_loader.py checks the same two properties), goes behind LAWFFT -- into
# ``Registry.more``, the tier behind ``rest``: tests/test_lawfft_loader.py holds ``rest`` and the end of ``order()`` to exactly those three.
internal_registry.add(GFISRArch(), more=True)
# GateRV3 likewise (tests/test_gaterv3_loader.py checks the same two properties), behind GFISR -- in ``Registry.beyond``, the tier behind
# ``more``: tests/test_gfisr_loader.py holds ``more`` to exactly GFISR and ``full()`` to ``order()`` + GFISR.  Later architectures of this
# kind go into ``beyond`` too.  The reference walks it right behind GateR.
internal_registry.add(GateRV3Arch(), beyond=True)
# GateRv2 likewise (tests/test_gaterv2_loader.py checks the same two properties), in ``beyond`` behind GateRV3: every older tier and iterator
# stays what it was.  The reference walks it between GateR and GateRV3.
internal_registry.add(GateRV2Arch(), beyond=True)
