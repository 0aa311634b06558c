"""Python-side builders for the C-ABI launch descriptors (no arithmetic happens here; the video-format and the still-image conversions at
the end also carry the f32 torch form of their definition for CPU tensors, as tiling._resample_frame does)."""

from __future__ import annotations

from dataclasses import dataclass

import torch

from . import lib as L
from .pack import pack_conv_weights, pad_bias  # noqa: F401  (pad_bias re-exported for the model files)
from .tensors import PF_BF16, PF_F16, Planes  # noqa: F401

_TORCH_TO_RSA = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16, torch.uint8: L.U8}


def rsa_dtype(dt: torch.dtype) -> int:
    try:
        return _TORCH_TO_RSA[dt]
    except KeyError:
        raise TypeError(f'resselt_amd supports float32/float16/bfloat16 tensors (and uint8 [N, H, W, C] images), got {dt}') from None


def current_stream_ptr(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def call(name: str, device, **kwargs) -> None:
    """One immediate C-ABI call by parameter name (``lib.call``) on ``device``'s current stream."""
    L.call(name, current_stream_ptr(device), **kwargs)


def require_cuda(x: torch.Tensor, what: str) -> None:
    """The engine has no CPU path: fail loudly instead of silently computing elsewhere."""
    if not x.is_cuda:
        raise RuntimeError(
            f'{what}: resselt_amd runs on MI355X HIP kernels only; got a tensor on {x.device}. '
            'Move the model and input to a cuda (ROCm) device.'
        )


def pack_weights_device(w: torch.Tensor, cin_planes: int, products: int, layout: int, fmt: int = PF_BF16) -> torch.Tensor:
    """OIHW f32 weights on the GPU -> packed A-fragment blob (``rsa_pack_weights``, one kernel; csrc/pack.hip).  The blob is returned as
    a bf16-typed tensor whatever ``fmt`` says: it is an opaque 16-bit container."""
    require_cuda(w, 'pack_weights')
    w = w.to(torch.float32).contiguous()
    cout, cin, k, _ = w.shape
    nbytes = int(L.load().rsa_packed_weight_bytes_layout(cout, cin_planes, k, products, layout))
    if nbytes <= 0:
        raise ValueError(f'unsupported convolution shape cout={cout} cin_planes={cin_planes} k={k} products={products}')
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w.device)
    with torch.cuda.device(w.device):
        call('rsa_pack_weights', w.device, w_oihw=w, cout=cout, cin=cin, cin_planes=cin_planes, ksize=k, products=products, layout=layout, fmt=fmt, out=out)
    return out


@dataclass
class ConvWeights:
    """One convolution's device-resident parameters.  ``packed`` is the blob in layout 0 (tap-major K order), or None when the
    weights are kept as f32 OIHW (``w``) and packed on demand in the layout the descriptor's schedule reads (``packed_for``)."""

    packed: torch.Tensor | None  # bf16 blob in layout 0, see pack.py / csrc/pack.hip
    bias: torch.Tensor  # f32, padded to 16
    cout: int
    cin: int
    cin_planes: int
    ksize: int
    products: int
    w: torch.Tensor | None = None  # f32 OIHW source on the device
    _by_layout: dict | None = None
    fmt: int = PF_BF16  # enum rsa_plane_fmt of the blob = of the input planes this layer multiplies

    @staticmethod
    def from_oihw(w: torch.Tensor, b: torch.Tensor | None, products: int, cin_planes: int | None = None, device=None, fmt: int | None = None) -> 'ConvWeights':
        """``products`` may be the module's ``Prec`` (an int that also names the plane format): ``fmt`` then defaults to it."""
        device = device if device is not None else w.device
        if fmt is None:
            fmt = getattr(products, 'fmt', PF_BF16)
        products = int(products)
        cout, cin, k, _ = w.shape
        if cin_planes is None:
            cin_planes = (cin + 7) // 8
        if cin > 8 * cin_planes:
            raise ValueError(f'cin={cin} does not fit in {cin_planes} planes')
        bias = pad_bias(None if b is None else b.to(device), cout, device)
        return ConvWeights(None, bias, cout, cin, cin_planes, k, products, w=w.detach().to(device=device, dtype=torch.float32).contiguous(), _by_layout={},
                           fmt=fmt)  # fmt: skip

    def packed_for(self, layout: int) -> torch.Tensor:
        if self.w is None:  # a blob written directly by a kernel (e.g. rsa_channel_attention_weights): layout 0 only
            if layout != 0:
                raise ValueError('pre-packed weights exist in layout 0 only')
            return self.packed
        blob = self._by_layout.get(layout)
        if blob is None:
            blob = self._by_layout[layout] = pack_weights_device(self.w, self.cin_planes, self.products, layout, self.fmt)
            if layout == 0:
                self.packed = blob
        return blob


def conv_params(
    wts: ConvWeights,
    x: Planes,
    H: int,
    W: int,
    *,
    in_plane0: int = 0,
    cin_planes: int | None = None,
    upsample2x: bool = False,
    act: int = L.ACT_NONE,
    act_param: float = 0.0,
    res1: 'torch.Tensor | tuple[Planes, int] | None' = None,
    alpha: float = 1.0,
    res2: 'torch.Tensor | tuple[Planes, int] | None' = None,
    beta: float = 1.0,
    out: Planes | None = None,
    out_plane_off: int = 0,
    out_f32: torch.Tensor | None = None,
    out_nchw: torch.Tensor | None = None,
    pixel_shuffle: int = 1,
    out_scale: float = 1.0,
    out_shift: torch.Tensor | None = None,
    act_vec: torch.Tensor | None = None,
    out_base: torch.Tensor | None = None,
    out_base_div: int = 0,
    out_lo8: bool = False,
    pool_sums: torch.Tensor | None = None,
) -> L.ConvParams:
    """Fill one ``rsa_conv_params``. ``H``, ``W`` are the OUTPUT size of the convolution."""
    p = L.ConvParams()
    p.batch = x.n
    p.H, p.W = H, W
    p.ksize = wts.ksize
    p.upsample2x = 1 if upsample2x else 0
    p.cin_planes = wts.cin_planes if cin_planes is None else cin_planes
    if p.cin_planes != wts.cin_planes:
        raise ValueError('cin_planes does not match the packed weights')
    p.cout = wts.cout
    p.products = wts.products
    exp_h, exp_w = (H // 2, W // 2) if upsample2x else (H, W)
    if (x.h, x.w) != (exp_h, exp_w):
        raise ValueError(f'input planes are {x.h}x{x.w}, expected {exp_h}x{exp_w}')
    if in_plane0 + p.cin_planes > x.planes:
        raise ValueError('input plane range exceeds the buffer')
    p.in_hi = x.hi_ptr(in_plane0)
    if x.fmt != wts.fmt:
        raise ValueError(f'input planes are in plane format {x.fmt} but the weights were packed for {wts.fmt}')
    p.in_fmt = wts.fmt
    if wts.products == 3:
        if not x.has_lo(in_plane0, p.cin_planes):
            raise ValueError('products=3 needs lo planes for every input plane')
        p.in_lo = x.lo_ptr(in_plane0)
    else:
        p.in_lo = None
    p.in_plane_stride = x.plane_stride
    p.in_batch_stride = x.batch_stride
    p.bias = wts.bias.data_ptr()
    p.act = act
    p.act_param = act_param
    p.alpha = alpha
    p.beta = beta
    p4 = (wts.cout + 3) // 4
    # a residual is an f32 map, or split planes given as (Planes, first plane): value = hi + lo
    # (a plane residual may carry a third element 'lo8': its lo halves are read from the buffer's 8-bit lo planes, rsa_conv_params.lo8_flags)
    plane_res = {}
    lo8_res = {}
    for name, r in (('res1', res1), ('res2', res2)):
        if isinstance(r, tuple):
            if len(r) == 3:
                if r[2] != 'lo8':
                    raise ValueError(f'{name}: the third element of a plane residual must be "lo8"')
                lo8_res[name] = True
                r = r[:2]
            pl, plane0 = r
            if (pl.n, pl.h, pl.w) != (x.n, H, W) or plane0 + (wts.cout + 7) // 8 > pl.planes or wts.cout % 8:
                raise ValueError(f'{name}: plane residual does not match the convolution output')
            plane_res[name] = (pl, plane0)
    if len({(pl.plane_stride, pl.batch_stride) for pl, _ in plane_res.values()}) > 1:
        raise ValueError('res1 and res2 plane residuals must share their strides')
    for name, r in (('res1', res1), ('res2', res2), ('out_f32', out_f32)):
        if r is not None and name not in plane_res:
            if tuple(r.shape) != (x.n, p4, H, W, 4) or r.dtype != torch.float32 or not r.is_contiguous():
                raise ValueError(f'{name} must be a contiguous f32 [N,{p4},{H},{W},4] map, got {tuple(r.shape)} {r.dtype}')
    p.res1 = None if res1 is None or 'res1' in plane_res else res1.data_ptr()
    p.res2 = None if res2 is None or 'res2' in plane_res else res2.data_ptr()
    if len({pl.fmt for pl, _ in plane_res.values()}) > 1:
        raise ValueError('res1 and res2 plane residuals must share their plane format')
    lo8_strides = set()
    for name, (pl, plane0) in plane_res.items():
        setattr(p, f'{name}_hi', pl.hi_ptr(plane0))
        if lo8_res.get(name):
            if pl.fmt != PF_F16 or not pl.has_lo8(plane0, (wts.cout + 7) // 8):
                raise ValueError(f'{name}: lo8 needs fp16 planes with an 8-bit lo buffer over the residual planes')
            setattr(p, f'{name}_lo', pl.lo8_ptr(plane0))
            p.lo8_flags |= L.LO8_RES1 if name == 'res1' else L.LO8_RES2
            lo8_strides.add(pl.lo8_batch_stride)
        else:
            setattr(p, f'{name}_lo', pl.lo_ptr(plane0) if pl.has_lo(plane0, (wts.cout + 7) // 8) else None)
        p.res_plane_stride, p.res_batch_stride = pl.plane_stride, pl.batch_stride
        p.res_fmt = pl.fmt
    p.out_f32 = None if out_f32 is None else out_f32.data_ptr()
    nplanes_out = (wts.cout + 7) // 8
    if out is not None:
        if (out.h, out.w, out.n) != (H, W, x.n) or out_plane_off + nplanes_out > out.planes:
            raise ValueError('output planes do not match the convolution output')
        p.out_hi = out.hi_ptr()
        # lo halves are written only where the buffer keeps them for EVERY plane this layer writes (see tensors.Planes.empty: lo_planes)
        if out_lo8:
            if out.fmt != PF_F16 or not out.has_lo8(out_plane_off, nplanes_out):
                raise ValueError('out_lo8 needs fp16 output planes with an 8-bit lo buffer over the written planes')
            p.out_lo = out.lo8_ptr()
            p.lo8_flags |= L.LO8_OUT
            lo8_strides.add(out.lo8_batch_stride)
        else:
            p.out_lo = out.lo_ptr() if out.has_lo(out_plane_off, nplanes_out) else None
        p.out_fmt = out.fmt
        p.out_plane_off = out_plane_off
        p.out_plane_stride = out.plane_stride
        p.out_batch_stride = out.batch_stride
    if out_lo8 and out is None:
        raise ValueError('out_lo8 without output planes')
    if p.lo8_flags:
        if len(lo8_strides) != 1:
            raise ValueError('the lo8 operands of a launch must share their batch stride')
        p.lo8_batch_stride = lo8_strides.pop()
    p.pixel_shuffle = pixel_shuffle
    p.out_scale = out_scale
    if out_nchw is not None:
        r = max(pixel_shuffle, 1)
        exp = (x.n, wts.cout // (r * r), H * r, W * r)
        if out_nchw.dtype == torch.uint8:  # 8-bit image, channel-interleaved
            exp = (x.n, H * r, W * r, wts.cout // (r * r))
        if tuple(out_nchw.shape) != exp or not out_nchw.is_contiguous():
            raise ValueError(f'out_nchw must be contiguous {exp}, got {tuple(out_nchw.shape)}')
        p.out_nchw = out_nchw.data_ptr()
        p.out_dtype = rsa_dtype(out_nchw.dtype)
        p.out_shift = None if out_shift is None else out_shift.data_ptr()
        if out_base is not None:
            if out_base.dim() != 4 or tuple(out_base.shape[:2]) != (x.n, exp[1]) or out_base.dtype != out_nchw.dtype or not out_base.is_contiguous():
                raise ValueError('out_base must be a contiguous [N, C_out, h, w] tensor of the output dtype')
            if out_base_div == 0 and tuple(out_base.shape[2:]) != (H, W):
                raise ValueError('out_base must be H x W unless out_base_div gives the nearest-upsampling factor')
            p.out_base = out_base.data_ptr()
            p.out_base_div, p.out_base_h, p.out_base_w = out_base_div, out_base.shape[2], out_base.shape[3]
    if act == L.ACT_PRELU:
        if act_vec is None or act_vec.numel() < ((wts.cout + 15) // 16) * 16 or act_vec.dtype != torch.float32:
            raise ValueError('PReLU needs f32 slopes padded to a multiple of 16')
        p.act_vec = act_vec.data_ptr()
    # the schedule this descriptor dispatches to decides the K order of the weight blob
    p.w_layout = int(L.load().rsa_conv_weight_layout(p))
    p.w_packed = wts.packed_for(p.w_layout).data_ptr()
    p.true_cin = min(wts.cin, 8 * p.cin_planes)  # python-side only (not part of the C struct): FLOP accounting in bench.py
    if pool_sums is not None:
        # per-channel partial sums of the f32 epilogue values (rsa_conv_params.pool_sums): f32 [N, slots, cout rounded up to 16]
        slots = conv_pool_slots(p)
        if slots is None:
            raise ValueError('pool_sums: the pooling epilogue is not compiled for this convolution (ask conv_pool_slots first)')
        exp = (x.n, slots, (wts.cout + 15) // 16 * 16)
        if tuple(pool_sums.shape) != exp or pool_sums.dtype != torch.float32 or not pool_sums.is_contiguous():
            raise ValueError(f'pool_sums must be a contiguous f32 {exp} tensor, got {tuple(pool_sums.shape)} {pool_sums.dtype}')
        p.pool_sums = pool_sums.data_ptr()
    return p


def conv_pool_slots(p: L.ConvParams) -> int | None:
    """Slots per image of ``pool_sums`` for this descriptor (``rsa_conv_pool_slots``), or None when the pooling epilogue is not compiled
    for it -- the caller then computes the mean some other way (``rsa_channel_gate``)."""
    rc = int(L.load().rsa_conv_pool_slots(p))
    if rc == L.E_UNSUPPORTED:
        return None
    if rc < 0:
        L.check(rc, 'rsa_conv_pool_slots')
    return rc


def run_convs(params: list[L.ConvParams], device) -> None:
    L.conv2d_list(params, current_stream_ptr(device))


def nchw_to_planes(x: torch.Tensor, out: Planes, mean: torch.Tensor | None = None, scale: float = 1.0, unshuffle: int = 1) -> None:  # noqa: C901
    """Plain [N,C,h,w] tensor -> split planes on the GPU (rsa_nchw_to_planes).

    ``out`` may be larger than ``x`` (up to 2x-1): the extra rows/columns are reflect-padded (SwinIR window padding).
    ``unshuffle=r`` fuses ``pixel_unshuffle(x, r)``: ``out`` is then the (H/r x W/r) grid with C*r*r channels.
    """
    require_cuda(x, 'nchw_to_planes')
    if not x.is_contiguous():
        x = x.contiguous()
    if x.dtype == torch.uint8:  # 8-bit image [N, H, W, C]: v = byte / 255 happens in the same kernel
        n, h, w, c = x.shape
    else:
        n, c, h, w = x.shape
    r = unshuffle
    if out.n != n or out.h * r < h or out.w * r < w or out.planes < (c * r * r + 7) // 8:
        raise ValueError('output planes do not match the input tensor')
    lo = out.lo_ptr() if out.has_lo(0, (c * r * r + 7) // 8) else None  # (lo halves only where every written plane carries them)
    call('rsa_nchw_to_planes', x.device, x=x, dtype=rsa_dtype(x.dtype), batch=n, C=c, H=out.h, W=out.w, src_h=h, src_w=w, unshuffle=r, mean=mean,
         scale=scale, out=out, out_lo=lo, out_fmt=out.fmt)  # fmt: skip


def planes_to_nchw(p: Planes, channels: int) -> torch.Tensor:
    """Split planes -> f32 [N,C,H,W] on the GPU (rsa_planes_to_nchw); for parity checks of intermediates."""
    out = torch.empty((p.n, channels, p.h, p.w), dtype=torch.float32, device=p.hi.device)
    call('rsa_planes_to_nchw', out.device, hi=p.hi_ptr(), lo=p.lo_ptr() if p.has_lo(0, (channels + 7) // 8) else None, plane_stride=p.plane_stride,
         batch_stride=p.batch_stride, batch=p.n, C=channels, H=p.h, W=p.w, fmt=p.fmt, out=out)  # fmt: skip
    return out


def image_u8_to_nchw(img: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """uint8 [N, H, W, C] image batch (or [H, W, C]) on the GPU -> float [N, C, H, W] in [0, 1] (rsa_image_u8_to_nchw)."""
    require_cuda(img, 'image_u8_to_nchw')
    if img.dtype != torch.uint8 or img.dim() not in (3, 4):
        raise TypeError(f'expected a uint8 [N, H, W, C] or [H, W, C] image, got {img.dtype} {tuple(img.shape)}')
    if img.dim() == 3:
        img = img.unsqueeze(0)
    img = img.contiguous()
    n, h, w, c = img.shape
    out = torch.empty((n, c, h, w), dtype=dtype, device=img.device)
    call('rsa_image_u8_to_nchw', img.device, img=img, batch=n, H=h, W=w, C=c, out=out, dtype=rsa_dtype(dtype))
    return out


def nchw_to_image_u8(x: torch.Tensor) -> torch.Tensor:
    """float [N, C, H, W] -> uint8 [N, H, W, C], ``(x.clamp(0, 1) * 255).round()`` (rsa_nchw_to_image_u8)."""
    require_cuda(x, 'nchw_to_image_u8')
    if x.dim() != 4:
        raise ValueError(f'expected a [N, C, H, W] tensor, got shape {tuple(x.shape)}')
    x = x.contiguous()
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, c), dtype=torch.uint8, device=x.device)
    call('rsa_nchw_to_image_u8', x.device, x=x, dtype=rsa_dtype(x.dtype), batch=n, C=c, H=h, W=w, img=out)
    return out


def tile_blend_accumulate(acc: torch.Tensor, y: torch.Tensor, window: tuple, src_offset: tuple, acc_offset: tuple, ramps: tuple) -> None:
    """Add the ``window = (rows, columns)`` of one tile's output ``y`` that starts at ``src_offset``, weighted by its ``ramps =
    (top, bottom, left, right)``, into the f32 ``[N, C, H, W]`` accumulator at ``acc_offset`` (``rsa_tile_blend_accumulate``: pixels in
    the top / left ramp are added to, all others stored).  ``y``: float ``[N, C, h, w]``, or a uint8 ``[N, h, w, C]`` image (code / 255)."""
    require_cuda(acc, 'tile_blend_accumulate')
    require_cuda(y, 'tile_blend_accumulate')
    if acc.dtype != torch.float32 or acc.dim() != 4 or not acc.is_contiguous():
        raise ValueError(f'the accumulator must be a contiguous float32 [N, C, H, W] tensor, got {acc.dtype} {tuple(acc.shape)}')
    if y.dim() != 4:
        raise ValueError(f'expected a [N, C, h, w] tensor or a uint8 [N, h, w, C] image, got shape {tuple(y.shape)}')
    y = y.contiguous()
    n, c, src_size = (y.shape[0], y.shape[3], (y.shape[1], y.shape[2])) if y.dtype == torch.uint8 else (y.shape[0], y.shape[1], (y.shape[2], y.shape[3]))
    if (n, c) != (acc.shape[0], acc.shape[1]):
        raise ValueError(f'tile output with batch {n} and {c} channels does not fit an accumulator of shape {tuple(acc.shape)}')
    L.tile_blend_accumulate(y.data_ptr(), rsa_dtype(y.dtype), n, c, window, src_size, src_offset, acc.data_ptr(), (acc.shape[2], acc.shape[3]),
                            acc_offset, ramps, current_stream_ptr(acc.device))  # fmt: skip


def _resample(x: torch.Tensor, size: tuple, filter: str, out_dtype: torch.dtype, what: str) -> torch.Tensor:
    """One launch of ``rsa_resample``: ``x`` (float ``[N, C, h, w]`` or a uint8 ``[N, h, w, C]`` image, code / 255) at ``size = (rows,
    columns)`` as ``out_dtype`` (uint8: an ``[N, rows, columns, C]`` image, ``clamp(0, 1) * 255`` rounded half to even)."""
    from ..tiling import resample_tables_device

    require_cuda(x, what)
    if x.dim() != 4:
        raise ValueError(f'expected a [N, C, h, w] tensor or a uint8 [N, h, w, C] image, got shape {tuple(x.shape)}')
    x = x.contiguous()
    n, c, (h, w) = (x.shape[0], x.shape[3], x.shape[1:3]) if x.dtype == torch.uint8 else (x.shape[0], x.shape[1], x.shape[2:4])
    oh, ow = (int(v) for v in size)
    (sy, wy), (sx, wx) = resample_tables_device(h, oh, filter, x.device), resample_tables_device(w, ow, filter, x.device)
    out = torch.empty((n, oh, ow, c) if out_dtype == torch.uint8 else (n, c, oh, ow), dtype=out_dtype, device=x.device)
    L.resample(x.data_ptr(), rsa_dtype(x.dtype), n, c, (h, w), out.data_ptr(), rsa_dtype(out_dtype), (oh, ow), (sy.data_ptr(), wy.data_ptr(), wy.shape[1]),
               (sx.data_ptr(), wx.data_ptr(), wx.shape[1]), current_stream_ptr(x.device))  # fmt: skip
    return out


def resample(x: torch.Tensor, size: tuple, filter: str = 'bicubic', dtype: torch.dtype | None = None) -> torch.Tensor:
    """``x`` (float ``[N, C, h, w]``, or a uint8 ``[N, h, w, C]`` image read as code / 255) resampled to ``size = (rows, columns)`` with
    torch's antialiased ``filter`` ('bicubic' or 'bilinear'; ``tiling.resample_table``): float ``[N, C, rows, columns]`` of ``dtype``
    (default: ``x``'s, float32 for an image).  One launch of ``rsa_resample``; at most 8 source pixels per output pixel along an axis."""
    if dtype is None:
        dtype = torch.float32 if x.dtype == torch.uint8 else x.dtype
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f'resample returns float32 / float16 / bfloat16 tensors, got dtype = {dtype}')
    return _resample(x, size, filter, dtype, 'resample')


def resample_to_image_u8(x: torch.Tensor, size: tuple, filter: str = 'bicubic') -> torch.Tensor:
    """As ``resample``, but the result is the uint8 ``[N, rows, columns, C]`` image ``(v.clamp(0, 1) * 255).round()``: resampling and the
    8-bit conversion of ``nchw_to_image_u8`` in one launch, rounded once."""
    return _resample(x, size, filter, torch.uint8, 'resample_to_image_u8')


# The pixel formats of video (csrc/yuv.hip): two-plane Y'CbCr 4:2:0.  The integers are the entry points' enums.
YUV_FORMATS = {'nv12': (8, torch.uint8), 'p010': (10, torch.uint16)}  # fmt -> (bits, dtype of the samples)
YUV_MATRICES = {'bt601': 0, 'bt709': 1, 'bt2020': 2}
YUV_RANGES = {'limited': 0, 'full': 1}
YUV_CHROMA_LOCS = {'left': 0, 'center': 1}
_YUV_KR_KB = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722), 'bt2020': (0.2627, 0.0593)}


def _yuv_args(fmt: str, matrix: str, range: str, chroma_loc: str) -> tuple:
    """``(bits, sample dtype)`` of ``fmt`` after every string has been checked (``ValueError`` names the bad one and the choices)."""
    for what, value, choices in (('fmt', fmt, YUV_FORMATS), ('matrix', matrix, YUV_MATRICES), ('range', range, YUV_RANGES), ('chroma_loc', chroma_loc, YUV_CHROMA_LOCS)):  # fmt: skip
        if value not in choices:
            raise ValueError(f'{what} = {value!r} is not one of {tuple(choices)}')
    return YUV_FORMATS[fmt]


def _yuv_planes(y: torch.Tensor, uv: torch.Tensor, fmt: str) -> tuple:
    """``y`` ``[H, W]`` / ``[N, H, W]`` and ``uv`` ``[H/2, W/2, 2]`` / ``[N, H/2, W/2, 2]`` as batched planes, checked against ``fmt``."""
    _, dt = YUV_FORMATS[fmt]
    if y.dim() not in (2, 3) or uv.dim() != y.dim() + 1:
        raise ValueError(f'expected y [H, W] or [N, H, W] and uv [H/2, W/2, 2] or [N, H/2, W/2, 2], got {tuple(y.shape)} and {tuple(uv.shape)}')
    if y.dtype != dt or uv.dtype != dt:
        raise ValueError(f'{fmt} planes are {dt}, got y {y.dtype} and uv {uv.dtype}')
    if y.dim() == 2:
        y, uv = y.unsqueeze(0), uv.unsqueeze(0)
    n, h, w = y.shape
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f'4:2:0 planes need an even, positive luma size, got {h} x {w}')
    if tuple(uv.shape) != (n, h // 2, w // 2, 2):
        raise ValueError(f'a y plane of shape {(n, h, w)} goes with a uv plane of shape {(n, h // 2, w // 2, 2)}, got {tuple(uv.shape)}')
    if y.device != uv.device:
        raise ValueError(f'y is on {y.device} and uv on {uv.device}')
    return y, uv


def _pitched(t: torch.Tensor, row_dims: int) -> tuple:
    """``(tensor, pitch, batch stride)`` in bytes of a batched plane whose rows are its last ``row_dims`` dimensions: a view whose rows are
    dense is passed as it is (its row stride is the pitch), anything else is made contiguous first."""
    dense = t.stride(-1) == 1 and (row_dims == 1 or t.stride(-2) == 2)
    row = t.shape[-1] * (t.shape[-2] if row_dims == 2 else 1)
    rows_dim = -1 - row_dims
    if not dense or t.stride(rows_dim) < row or (t.shape[0] > 1 and t.stride(0) < t.stride(rows_dim) * t.shape[rows_dim]):
        t = t.contiguous()
    return t, t.stride(rows_dim) * t.element_size(), t.stride(0) * t.element_size()


def _yuv_coefficients(matrix: str, range: str, bits: int) -> tuple:
    """``(Kr, Kg, Kb, luma offset, luma range, chroma offset, chroma range)`` in codes, as Python floats."""
    kr, kb = _YUV_KR_KB[matrix]
    m, top = 2 ** (bits - 8), 2**bits - 1
    if range == 'limited':
        return kr, 1.0 - kr - kb, kb, 16.0 * m, 219.0 * m, 128.0 * m, 224.0 * m
    return kr, 1.0 - kr - kb, kb, 0.0, float(top), float(2 ** (bits - 1)), float(top)


def _codes(t: torch.Tensor, bits: int) -> torch.Tensor:
    """The samples of a plane as f32 codes (P010: the top 10 bits of the word)."""
    c = t.to(torch.int32)
    return (c >> 6 if bits == 10 else c).to(torch.float32)


def _chroma_up(c: torch.Tensor, dim: int, n: int, o: float) -> torch.Tensor:
    """Axis ``dim`` of the chroma codes ``c`` interpolated linearly to ``n`` luma positions for the siting offset ``o`` (exact in f32)."""
    u = (torch.arange(n, dtype=torch.float64, device=c.device) - o) / 2
    j = torch.floor(u)
    f = (u - j).to(torch.float32)
    last = c.shape[dim] - 1
    j = j.to(torch.int64)
    shape = [1] * c.dim()
    shape[dim] = n
    f = f.reshape(shape)
    return (1 - f) * c.index_select(dim, j.clamp(0, last)) + f * c.index_select(dim, (j + 1).clamp(0, last))


def _yuv420_to_nchw_torch(y, uv, bits, matrix, range, chroma_loc, dtype):
    """``yuv420_to_nchw`` for CPU tensors: the definition of csrc/yuv.hip in f32 torch operations (on whatever device the planes are: on the
    GPU it is the chain of torch operations a caller needed before the kernel existed, which tools/yuv_measure.py times)."""
    kr, kg, kb, y_off, y_range, c_off, c_range = _yuv_coefficients(matrix, range, bits)
    n, h, w = y.shape
    c = _chroma_up(_codes(uv, bits), 1, h, 0.5)
    c = _chroma_up(c, 2, w, 0.5 if chroma_loc == 'center' else 0.0)
    yn = (_codes(y, bits) - y_off) * (1.0 / y_range)
    cb, cr = (c[..., 0] - c_off) * (1.0 / c_range), (c[..., 1] - c_off) * (1.0 / c_range)
    r = yn + (2 * (1 - kr)) * cr
    b = yn + (2 * (1 - kb)) * cb
    g = yn - (kb * 2 * (1 - kb) / kg) * cb - (kr * 2 * (1 - kr) / kg) * cr
    return torch.stack((r, g, b), 1).clamp(0, 1).to(dtype)


def _chroma_down(d: torch.Tensor, dim: int, o: float) -> torch.Tensor:
    """The SUM (2 terms for ``o = 0.5``, [1 2 1] for ``o = 0``; the caller divides) that makes one chroma sample of every two luma positions."""
    n = d.shape[dim]
    even = torch.arange(0, n, 2, device=d.device)
    if o == 0.5:
        return d.index_select(dim, even) + d.index_select(dim, even + 1)
    return (d.index_select(dim, (even - 1).clamp(min=0)) + 2 * d.index_select(dim, even)) + d.index_select(dim, even + 1)


def _nchw_to_yuv420_torch(x, bits, dt, matrix, range, chroma_loc):
    """``nchw_to_yuv420`` for CPU tensors: the definition of csrc/yuv.hip in f32 torch operations."""
    kr, kg, kb, y_off, y_range, c_off, c_range = _yuv_coefficients(matrix, range, bits)
    v = x.to(torch.float32)
    v = torch.where(v.isnan(), torch.zeros_like(v), v).clamp(0, 1)
    r, g, b = v[:, 0], v[:, 1], v[:, 2]
    yn = kr * r + (kg * g + kb * b)
    top = float(2**bits - 1)

    def codes(t):
        t = t.round().clamp(0, top).to(torch.int32)  # torch rounds half to even
        return (t << 6 if bits == 10 else t).to(dt)

    y = codes(yn * y_range + y_off)
    center = chroma_loc == 'center'
    filt = 0.25 if center else 0.125
    planes = []
    for d, k in ((b - yn, kb), (r - yn, kr)):
        s = _chroma_down(_chroma_down(d, 1, 0.5), 2, 0.5 if center else 0.0)
        planes.append(codes(s * (c_range * filt / (2 * (1 - k))) + c_off))
    return y, torch.stack(planes, -1)


def yuv420_to_nchw(y: torch.Tensor, uv: torch.Tensor, fmt: str = 'nv12', matrix: str = 'bt709', range: str = 'limited', chroma_loc: str = 'left',
                   dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """A two-plane Y'CbCr 4:2:0 frame -> float ``[N, 3, H, W]`` R'G'B' in [0, 1] of ``dtype`` (``rsa_yuv420_to_nchw``, one launch).

    ``y``: ``[H, W]`` or ``[N, H, W]``; ``uv``: ``[H/2, W/2, 2]`` or ``[N, H/2, W/2, 2]`` interleaved (Cb, Cr); ``torch.uint8`` for
    ``fmt = 'nv12'``, ``torch.uint16`` words with the code in their top 10 bits for ``'p010'``.  A row-strided view (a pitched decoder
    surface: innermost stride 1) is read in place, its row stride is the pitch.  ``matrix``: 'bt601' / 'bt709' / 'bt2020' (non-constant
    luminance); ``range``: 'limited' / 'full'; ``chroma_loc``: 'left' (H.264 / HEVC default) or 'center'.  Chroma is interpolated
    linearly, the result is clamped to [0, 1]; the transfer function is untouched.  CPU tensors take the same definition in f32 torch."""
    bits, _ = _yuv_args(fmt, matrix, range, chroma_loc)
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f'yuv420_to_nchw returns float32 / float16 / bfloat16 tensors, got dtype = {dtype}')
    y, uv = _yuv_planes(y, uv, fmt)
    if not y.is_cuda:
        return _yuv420_to_nchw_torch(y, uv, bits, matrix, range, chroma_loc, dtype)
    (y, y_pitch, y_stride), (uv, uv_pitch, uv_stride) = _pitched(y, 1), _pitched(uv, 2)
    n, h, w = y.shape
    out = torch.empty((n, 3, h, w), dtype=dtype, device=y.device)
    with torch.cuda.device(y.device):
        L.yuv420_to_nchw((y.data_ptr(), y_pitch, y_stride), (uv.data_ptr(), uv_pitch, uv_stride), bits, n, (h, w), YUV_MATRICES[matrix],
                         YUV_RANGES[range], YUV_CHROMA_LOCS[chroma_loc], out.data_ptr(), rsa_dtype(dtype), current_stream_ptr(y.device))  # fmt: skip
    return out


def nchw_to_yuv420(x: torch.Tensor, fmt: str = 'nv12', matrix: str = 'bt709', range: str = 'limited', chroma_loc: str = 'left') -> tuple:
    """Float ``[N, 3, H, W]`` R'G'B' -> the contiguous planes ``(y [N, H, W], uv [N, H/2, W/2, 2])`` of ``fmt`` (``rsa_nchw_to_yuv420``: both
    planes from one launch).  The source is clamped to [0, 1] (NaN -> 0), Cb and Cr are filtered to the ``chroma_loc`` siting ([1 2 1] / 4
    or the mean of two, per axis), codes are rounded half to even.  Arguments as ``yuv420_to_nchw``; CPU tensors take f32 torch."""
    bits, dt = _yuv_args(fmt, matrix, range, chroma_loc)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f'expected a [N, 3, H, W] tensor, got shape {tuple(x.shape)}')
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f'nchw_to_yuv420 reads float32 / float16 / bfloat16 tensors, got {x.dtype}')
    n, _, h, w = x.shape
    if h < 2 or w < 2 or h % 2 or w % 2:
        raise ValueError(f'4:2:0 planes need an even, positive frame size, got {h} x {w}')
    if not x.is_cuda:
        return _nchw_to_yuv420_torch(x, bits, dt, matrix, range, chroma_loc)
    x = x.contiguous()
    y = torch.empty((n, h, w), dtype=dt, device=x.device)
    uv = torch.empty((n, h // 2, w // 2, 2), dtype=dt, device=x.device)
    e = y.element_size()
    with torch.cuda.device(x.device):
        L.nchw_to_yuv420(x.data_ptr(), rsa_dtype(x.dtype), n, (h, w), YUV_MATRICES[matrix], YUV_RANGES[range], YUV_CHROMA_LOCS[chroma_loc], bits,
                         (y.data_ptr(), w * e, h * w * e), (uv.data_ptr(), w * e, (h // 2) * w * e), current_stream_ptr(x.device))  # fmt: skip
    return y, uv


# The still-image formats of upscale_rgba (csrc/rgba.hip): interleaved images of 1 .. 4 channels, 8 or 16 bits.
IMAGE_DEPTHS = {8: torch.uint8, 16: torch.uint16}
ALPHA_MODES = {'none': 0, 'model': 1, 'resample': 2}  # the entry point's alpha_mode
MAX_BLEED = 16


def _image_args(img: torch.Tensor, what: str) -> tuple:
    """``(batched image, bits)`` of an interleaved ``[H, W, C]`` / ``[N, H, W, C]`` image, checked (``ValueError``)."""
    if img.dtype not in (torch.uint8, torch.uint16):
        raise ValueError(f'{what}: an image is torch.uint8 or torch.uint16, got {img.dtype}')
    if img.dim() not in (3, 4):
        raise ValueError(f'{what}: expected an [H, W, C] or [N, H, W, C] image, got shape {tuple(img.shape)}')
    if img.dim() == 3:
        img = img.unsqueeze(0)
    n, h, w, c = img.shape
    if not 1 <= c <= 4 or n < 1 or h < 1 or w < 1:
        raise ValueError(f'{what}: an image has 1 (gray), 2 (gray + alpha), 3 (RGB) or 4 (RGBA) channels and a positive size, got shape {tuple(img.shape)}')
    return img, 8 if img.dtype == torch.uint8 else 16


def _check_bleed(bleed) -> int:
    if isinstance(bleed, bool) or int(bleed) != bleed or not 0 <= bleed <= MAX_BLEED:
        raise ValueError(f'bleed = {bleed} must be an integer in 0 .. {MAX_BLEED}')
    return int(bleed)


def _pitched_image(img: torch.Tensor) -> tuple:
    """``(image, pitch, batch stride)`` in bytes of an ``[N, H, W, C]`` image: a view whose pixels and rows are dense (innermost strides
    ``C`` and 1) is passed as it is, its row stride is the pitch; anything else is made contiguous first."""
    n, h, w, c = img.shape
    if img.stride(3) != 1 or img.stride(2) != c or img.stride(1) < w * c or (n > 1 and img.stride(0) < img.stride(1) * h):
        img = img.contiguous()
    e = img.element_size()
    return img, img.stride(1) * e, img.stride(0) * e


def _bleed_torch(col: torch.Tensor, known: torch.Tensor, passes: int) -> torch.Tensor:
    """The edge bleed of csrc/rgba.hip on f32 ``col`` ``[N, Cs, H, W]`` with ``known`` bool ``[N, 1, H, W]``: f32 sums in row-major order
    over the 3 x 3 (a term outside S adds an exact zero)."""
    import torch.nn.functional as F

    h, w = col.shape[2:]
    for _ in range(passes):
        if bool(known.all()) or not bool(known.any()):
            break
        cp, kp = F.pad(col * known, (1, 1, 1, 1)), F.pad(known.to(torch.float32), (1, 1, 1, 1))
        num, den = torch.zeros_like(col), torch.zeros_like(kp[:, :, 1:-1, 1:-1])
        for dy in range(3):
            for dx in range(3):
                if (dy, dx) != (1, 1):
                    wgt = 2.0 if dy == 1 or dx == 1 else 1.0
                    num = num + wgt * cp[:, :, dy : dy + h, dx : dx + w]
                    den = den + wgt * kp[:, :, dy : dy + h, dx : dx + w]
        fill = ~known & (den > 0)
        col = torch.where(fill, num / den.clamp(min=1.0), col)
        known = known | fill
    return col


def image_to_nchw_alpha(img: torch.Tensor, model_channels: int = 3, alpha: str = 'model', bleed: int = 8, dtype: torch.dtype = torch.float16) -> tuple:
    """An interleaved image -> ``(x, a, flags)`` for a model of ``model_channels`` (``rsa_image_to_nchw_alpha``, one launch).

    ``img``: ``[H, W, C]`` or ``[N, H, W, C]``, ``torch.uint8`` or ``torch.uint16`` (full range), ``C`` = 1 gray, 2 gray + alpha, 3 RGB,
    4 RGBA; alpha is straight.  A row-strided view whose innermost two strides are dense is read in place.  Values are ``code / M``
    (``M`` = 255 or 65535); gray is replicated to ``model_channels`` = 3; a colour image needs 3.  The colour under ``alpha = 0`` pixels
    is bled in from the visible edge in ``bleed`` (0 .. 16) passes (csrc/rgba.hip has the definition); alpha itself never changes.
    ``x`` is ``[N, Cm, H, W]`` of ``dtype``; with ``alpha = 'model'`` on an image with an alpha channel it is ``[2 N, Cm, H, W]``: the
    alpha, replicated to ``Cm`` channels, sits behind the colour entries.  ``a`` is the f32 ``[N, 1, H, W]`` alpha for
    ``alpha = 'resample'``, else None.  ``flags`` is int32 ``[N]``: 1 where an alpha code of the image is below the maximum (None for
    images without alpha, which ignore ``alpha`` and ``bleed``).  CPU tensors take the same definition in f32 torch."""
    img, bits = _image_args(img, 'image_to_nchw_alpha')
    bleed = _check_bleed(bleed)
    if alpha not in ALPHA_MODES:
        raise ValueError(f'alpha = {alpha!r} is not one of {tuple(ALPHA_MODES)}')
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f'image_to_nchw_alpha returns float32 / float16 / bfloat16 tensors, got dtype = {dtype}')
    n, h, w, c = img.shape
    cm = int(model_channels)
    if cm not in (1, 3) or (c >= 3 and cm != 3):
        raise ValueError(f'an image of {c} channels needs a model of 3 channels (gray: 1 or 3), got {model_channels}')
    has_alpha = c in (2, 4)
    mode = ALPHA_MODES[alpha] if has_alpha else 0
    if not img.is_cuda:
        m = 255.0 if bits == 8 else 65535.0
        codes = img.to(torch.int32).permute(0, 3, 1, 2)
        col = codes[:, : c - has_alpha].to(torch.float32) / m
        a = flags = None
        if has_alpha:
            ac = codes[:, c - 1 :]
            col = _bleed_torch(col, ac > 0, bleed)
            flags = (ac.reshape(n, -1) < int(m)).any(1).to(torch.int32)
            av = ac.to(torch.float32) / m
        x = col.expand(n, cm, h, w).to(dtype) if col.shape[1] == 1 else col.to(dtype)
        if mode == 1:
            x = torch.cat((x, av.expand(n, cm, h, w).to(dtype)))
        elif mode == 2:
            a = av.contiguous()
        return x.contiguous(), a, flags
    img, pitch, stride = _pitched_image(img)
    x = torch.empty(((2 * n if mode == 1 else n), cm, h, w), dtype=dtype, device=img.device)
    a = torch.empty((n, 1, h, w), dtype=torch.float32, device=img.device) if mode == 2 else None
    flags = torch.zeros(n, dtype=torch.int32, device=img.device) if has_alpha else None
    with torch.cuda.device(img.device):
        L.image_to_nchw_alpha((img.data_ptr(), pitch, stride), bits, n, (h, w), c, cm, bleed if has_alpha else 0, x.data_ptr(), rsa_dtype(dtype),
                              x[n:].data_ptr() if mode == 1 else (a.data_ptr() if mode == 2 else None), mode,
                              flags.data_ptr() if has_alpha else None, current_stream_ptr(img.device))  # fmt: skip
    return x, a, flags


def nchw_to_image_alpha(color: torch.Tensor, alpha: torch.Tensor | None = None, channels: int = 3, bits: int = 8) -> torch.Tensor:
    """Float colour ``[N, Cm, H, W]`` (and an alpha source ``[N, Ca, H, W]``, ``Ca`` = 1 or ``Cm``, or None) -> the contiguous interleaved
    ``[N, H, W, channels]`` image of ``bits`` = 8 (uint8) or 16 (uint16) (``rsa_nchw_to_image_alpha``, one launch).  Gray
    (``channels`` = 1, 2) is the f32 mean of the ``Cm`` colour channels, alpha (``channels`` = 2, 4) the f32 mean of the alpha source's
    channels, or the maximum code without one; each value is clamped to [0, 1] (NaN -> 0), multiplied by 255 / 65535 and rounded half
    to even.  CPU tensors take the same definition in f32 torch."""
    if bits not in IMAGE_DEPTHS:
        raise ValueError(f'bits = {bits} must be 8 or 16')
    c = int(channels)
    if not 1 <= c <= 4:
        raise ValueError(f'channels = {channels} must be 1 .. 4')
    if color.dim() != 4 or color.shape[1] not in (1, 3) or (c >= 3 and color.shape[1] != 3):
        raise ValueError(f'expected a [N, 1 or 3, H, W] colour tensor (3 for a colour image), got shape {tuple(color.shape)}')
    n, cm, h, w = color.shape
    if c in (1, 3):
        alpha = None
    for t, what in ((color, 'colour'), (alpha, 'alpha')):
        if t is not None and t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f'nchw_to_image_alpha reads float32 / float16 / bfloat16 tensors, got {t.dtype} ({what})')
    if alpha is not None and (alpha.dim() != 4 or alpha.shape[1] not in (1, cm) or (alpha.shape[0], *alpha.shape[2:]) != (n, h, w) or alpha.device != color.device):
        raise ValueError(f'the alpha source of a colour tensor of shape {tuple(color.shape)} is [N, 1 or {cm}, H, W] on the same device, got {tuple(alpha.shape)}')
    dt = IMAGE_DEPTHS[bits]
    if not color.is_cuda:
        m = 255.0 if bits == 8 else 65535.0

        def mean(t):
            t = t.to(torch.float32)
            return ((t[:, 0] + t[:, 1]) + t[:, 2]) / 3.0 if t.shape[1] == 3 else t[:, 0]

        planes = [mean(color)] if c <= 2 else [color[:, i].to(torch.float32) for i in range(3)]
        if c in (2, 4):
            planes.append(mean(alpha) if alpha is not None else torch.ones((n, h, w), dtype=torch.float32))
        v = torch.stack(planes, -1)
        v = torch.where(v.isnan(), torch.zeros_like(v), v).clamp(0, 1)
        return (v * m).round().to(torch.int32).to(dt).contiguous()  # torch rounds half to even
    color = color.contiguous()
    alpha = None if alpha is None else alpha.contiguous()
    out = torch.empty((n, h, w, c), dtype=dt, device=color.device)
    e = out.element_size()
    with torch.cuda.device(color.device):
        L.nchw_to_image_alpha(color.data_ptr(), rsa_dtype(color.dtype), cm, None if alpha is None else alpha.data_ptr(),
                              L.F32 if alpha is None else rsa_dtype(alpha.dtype), 1 if alpha is None else alpha.shape[1], n, (h, w), c, bits,
                              (out.data_ptr(), w * c * e, h * w * c * e), current_stream_ptr(color.device))  # fmt: skip
    return out
