"""Operator-level Python entry points over the C ABI (torch CUDA tensors are containers only).

Each function names the reference op it stands in for; argument meaning and error behaviour follow
that op.  Tensors must be fp32, contiguous (unless a stride argument exists) and on a HIP device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import Epilogue, check, ptr, stream_ptr

_ROPE_CACHE = {}


def _req(t: torch.Tensor, name: str):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"{name} must be a contiguous float32 CUDA tensor")
    return t


def rope_tables(device, base: float = 100.0, max_pos: int = 256):
    """cos/sin [max_pos, 16] on `device`, computed by the library like RoPE2D.get_cos_sin (pos_embed.py:118-128)."""
    key = (str(device), float(base), max_pos)
    if key not in _ROPE_CACHE:
        cos = np.empty((max_pos, 16), np.float32)
        sin = np.empty((max_pos, 16), np.float32)
        check(_lib.load().a3r_rope_table_host(cos.ctypes.data_as(C.c_void_p), sin.ctypes.data_as(C.c_void_p), max_pos, base))
        _ROPE_CACHE[key] = (torch.from_numpy(cos).to(device), torch.from_numpy(sin).to(device))
    return _ROPE_CACHE[key]


def rope_2d(tokens: torch.Tensor, positions: torch.Tensor, base: float, fwd: float = 1.0):
    """curope.rope_2d(tokens[B,N,H,D], positions[B,N,2] int64, base, fwd): in place (curope.cpp:49-65)."""
    if tokens.dim() != 4:
        raise RuntimeError("tokens must have 4 dimensions")
    if positions.dim() != 3:
        raise RuntimeError("positions must have 3 dimensions")
    if tokens.size(0) != positions.size(0):
        raise RuntimeError("batch size differs between tokens & positions")
    if tokens.size(1) != positions.size(1):
        raise RuntimeError("seq_length differs between tokens & positions")
    if positions.size(2) != 2:
        raise RuntimeError("positions.shape[2] must be equal to 2")
    if tokens.is_cuda != positions.is_cuda:
        raise RuntimeError("tokens and positions are not on the same device")
    _req(tokens, "tokens")
    if positions.dtype != torch.int64 or not positions.is_contiguous():
        raise RuntimeError("positions must be a contiguous int64 tensor")
    B, N, H, D = tokens.shape
    check(_lib.load().a3r_rope2d(ptr(tokens), ptr(positions), B, N, H, D, base, fwd, stream_ptr()), "rope_2d")
    return tokens


def layernorm(x, w, b, eps=1e-6, out=None):
    """nn.LayerNorm over the last dim."""
    _req(x, "x")
    D = x.shape[-1]
    M = x.numel() // D
    out = torch.empty_like(x) if out is None else out
    check(_lib.load().a3r_layernorm(ptr(x), ptr(_req(w, "w")), ptr(_req(b, "b")), ptr(out), M, D, eps, stream_ptr()), "layernorm")
    return out


def make_epilogue(kind=_lib.EPI_NONE, bias=None, resid=None, resid2=None, relu_a=False, rope=None, pixshuf=None, out_bf3=False,
                  aux_bf3=None, aux_relu=False, out_pair=False, out_fh2=False, aux_fh2=None, x_scale=0.0, out_scale=0.0, out_absmax=None,
                  head=None, relu_out=False, relu_acc=False):
    e = Epilogue()
    e.relu_out, e.relu_acc = int(relu_out), int(relu_acc)
    if head is not None:              # EPI_HEAD: (head_w [4, 128], head_b [4], conf out [M]) -- the caller keeps them alive
        e.head_w, e.head_b, e.head_conf = head[0].data_ptr(), head[1].data_ptr(), head[2].data_ptr()
    # range control of the fh2 kernels (include/a3r.h): zeros / None = scale 1, no statistics
    e.x_scale, e.out_scale = float(x_scale), float(out_scale)
    e.out_absmax = None if out_absmax is None else out_absmax.data_ptr()
    e.out_fh2 = int(out_fh2)
    e.aux_fh2 = None if aux_fh2 is None else aux_fh2.data_ptr()
    e.out_bf3 = int(out_bf3)
    e.out_pair = int(out_pair)
    e.aux_bf3 = None if aux_bf3 is None else aux_bf3.data_ptr()
    e.aux_relu = int(aux_relu)
    e.epi = kind
    e.bias = None if bias is None else bias.data_ptr()
    e.resid = None if resid is None else resid.data_ptr()
    e.resid2 = None if resid2 is None else resid2.data_ptr()
    e.relu_a = int(relu_a)
    if rope is not None:
        e.rope_cols, e.tokens_per_image, e.grid_w, cos, sin = rope
        e.rope_cos, e.rope_sin = cos.data_ptr(), sin.data_ptr()
    if pixshuf is not None:
        e.ps_s, e.ps_h, e.ps_w, e.ps_cout = pixshuf
    return e


def linear(x, w, bias=None, epi=_lib.EPI_NONE, out=None, **kw):
    """nn.Linear on x [..., K] with w [N, K] (+ fused epilogue, see include/a3r.h)."""
    _req(x, "x"); _req(w, "w")
    K = x.shape[-1]
    M = x.numel() // K
    N = w.shape[0]
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=torch.float32)
    e = make_epilogue(epi, bias, **kw)
    check(_lib.load().a3r_linear(ptr(x), K, ptr(w), ptr(out), out.shape[-1] if epi != _lib.EPI_PIXSHUF else e.ps_cout,
                                 M, N, K, C.byref(e), stream_ptr()), "linear")
    return out


def linear_grouped(xs, ws, biases, epi=_lib.EPI_NONE, resids=None, **kw):
    """Several same-shape nn.Linear problems in one launch (a3r_linear_grouped)."""
    G = len(xs)
    K = xs[0].shape[-1]
    M = xs[0].numel() // K
    N = ws[0].shape[0]
    outs = [torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=torch.float32) for x in xs]
    arr = (_lib.GroupPtrs * G)()
    for i in range(G):
        _req(xs[i], "x"); _req(ws[i], "w")
        arr[i].x, arr[i].w, arr[i].y = xs[i].data_ptr(), ws[i].data_ptr(), outs[i].data_ptr()
        arr[i].bias = None if biases is None else biases[i].data_ptr()
        arr[i].resid = None if resids is None else resids[i].data_ptr()
    e = make_epilogue(epi, **kw)
    check(_lib.load().a3r_linear_grouped(arr, G, K, N, M, N, K, C.byref(e), stream_ptr()), "linear_grouped")
    return outs


def bf3_set_products(n: int) -> int:
    """Arithmetic mode of the bf3 kernels: 6 (fp32-accurate, default), 3 or 1 (plain bf16 operands).  Returns the previous mode."""
    return int(_lib.load().a3r_bf3_set_products(int(n)))


def fh2_set_passes(n: int) -> int:
    """Arithmetic mode of the fh2 kernels: 3 (fp32-grade, default) or 1 (plain fp16 operands).  Returns the previous mode."""
    return int(_lib.load().a3r_fh2_set_passes(int(n)))


class Bf3:
    """An fp32 matrix [rows, K] in bf3 form (three exact bf16 planes, include/a3r.h): uint8 storage + logical shape."""

    def __init__(self, data: torch.Tensor, rows: int, K: int, weight: bool = False):
        self.data, self.rows, self.K, self.weight = data, rows, K, weight          # weight: the row-pair layout (include/a3r.h)

    def data_ptr(self):
        return self.data.data_ptr()

    def planes(self):
        """-> float32 [3, rows, K]: the three planes (their sum is the original matrix exactly)."""
        if self.weight:        # [ceil(rows/2)][K/32][2][4][3][8] -> rows-major
            u = self.data.view(torch.int16).view(-1, self.K // 32, 2, 4, 3, 8).permute(0, 2, 1, 3, 4, 5)
            u = u.reshape(-1, self.K // 8, 3, 8)[:self.rows].to(torch.int32) << 16
        else:
            u = self.data.view(torch.int16).view(self.rows, self.K // 8, 3, 8).to(torch.int32) << 16
        return u.view(torch.float32).permute(2, 0, 1, 3).reshape(3, self.rows, self.K)


def split_bf3(x) -> Bf3:
    """fp32 x [..., K] -> bf3 (a3r_split_bf3)."""
    _req(x, "x")
    K = x.shape[-1]
    M = x.numel() // K
    y = torch.empty(M * K * 6, device=x.device, dtype=torch.uint8)
    check(_lib.load().a3r_split_bf3(ptr(x), K, ptr(y), M, K, stream_ptr()), "split_bf3")
    return Bf3(y, M, K)


def split_bf3_w(w) -> Bf3:
    """fp32 weights [N, K] -> bf3 in the row-pair weight layout (a3r_split_bf3_w): the w3 / wp3 operand of linear_bf3 / conv3x3_bf3."""
    _req(w, "w")
    N, K = w.shape
    lib = _lib.load()
    y = torch.zeros(int(lib.a3r_bf3_w_bytes(N, K)), device=w.device, dtype=torch.uint8)
    check(lib.a3r_split_bf3_w(ptr(w), K, ptr(y), N, K, stream_ptr()), "split_bf3_w")
    return Bf3(y, N, K, weight=True)


def _need_weight_layout(w3, who):
    if not w3.weight:
        raise RuntimeError(f"{who}: the weight operand must be in the row-pair weight layout (ops.split_bf3_w)")


def layernorm_bf3(x, w, b, eps=1e-6, pair=False) -> Bf3:
    """nn.LayerNorm over the last dim with the output written in bf3 form (a3r_layernorm_bf3); pair: in the row-pair layout."""
    _req(x, "x")
    D = x.shape[-1]
    M = x.numel() // D
    y = torch.zeros((M + (M & 1 if pair else 0)) * D * 6, device=x.device, dtype=torch.uint8)      # row pairs: an even number of rows
    check(_lib.load().a3r_layernorm_bf3(ptr(x), ptr(_req(w, "w")), ptr(_req(b, "b")), ptr(y), M, D, eps, int(pair), stream_ptr()), "layernorm_bf3")
    return Bf3(y, M, D, weight=bool(pair))


def linear_bf3(x3: Bf3, w3: Bf3, bias=None, epi=_lib.EPI_NONE, out=None, **kw):
    """nn.Linear on the bf16 matrix cores with fp32 accuracy: x3 [M, K], w3 [N, K] in bf3 form (a3r_linear_bf3)."""
    M, K, N = x3.rows, x3.K, w3.rows
    _need_weight_layout(w3, "linear_bf3")
    if w3.K != K:
        raise RuntimeError(f"linear_bf3: K mismatch ({K} vs {w3.K})")
    e = make_epilogue(epi, bias, **kw)
    e.x_pair = int(x3.weight)
    if e.out_bf3:          # y in bf3 form, for the next bf3 GEMM
        y3 = Bf3(torch.zeros((M + (M & 1 if e.out_pair else 0)) * N * 6, device=x3.data.device, dtype=torch.uint8), M, N, weight=bool(e.out_pair))
        check(_lib.load().a3r_linear_bf3(x3.data_ptr(), w3.data_ptr(), y3.data_ptr(), N, M, N, K, C.byref(e), stream_ptr()), "linear_bf3")
        return y3
    if out is None:
        out = torch.empty((M, N), device=x3.data.device, dtype=torch.float32)
    check(_lib.load().a3r_linear_bf3(x3.data_ptr(), w3.data_ptr(), ptr(out), out.shape[-1] if epi != _lib.EPI_PIXSHUF else e.ps_cout,
                                     M, N, K, C.byref(e), stream_ptr()), "linear_bf3")
    return out


def linear_bf3_grouped(x3s, w3s, biases, epi=_lib.EPI_NONE, resids=None, **kw):
    """Several same-shape bf3 nn.Linear problems in one launch (a3r_linear_bf3_grouped)."""
    G = len(x3s)
    M, K, N = x3s[0].rows, x3s[0].K, w3s[0].rows
    for w3 in w3s:
        _need_weight_layout(w3, "linear_bf3_grouped")
    outs = [torch.empty((M, N), device=x3s[0].data.device, dtype=torch.float32) for _ in range(G)]
    arr = (_lib.GroupPtrs * G)()          # same field layout as a3r_group_ptrs_bf3
    for i in range(G):
        arr[i].x, arr[i].w, arr[i].y = x3s[i].data_ptr(), w3s[i].data_ptr(), outs[i].data_ptr()
        arr[i].bias = None if biases is None else biases[i].data_ptr()
        arr[i].resid = None if resids is None else resids[i].data_ptr()
    e = make_epilogue(epi, **kw)
    e.x_pair = int(x3s[0].weight)
    check(_lib.load().a3r_linear_bf3_grouped(arr, G, N, M, N, K, C.byref(e), stream_ptr()), "linear_bf3_grouped")
    return outs


def conv3x3_bf3(x3: Bf3, wp3: Bf3, shape, bias=None, stride=1, epi=_lib.EPI_NONE, **kw):
    """3x3 conv (padding 1) on the bf3 kernel: x3 = bf3 of the channels-last map `shape` = (B, H, W, Cin), wp3 = bf3 of the
    packed weights [Cout, 9 Cin].  Returns fp32 [B, Ho, Wo, Cout] (or a Bf3 with out_bf3=True)."""
    B, H, W, Cin = shape
    Cout = wp3.rows
    _need_weight_layout(wp3, "conv3x3_bf3")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    e = make_epilogue(epi, bias, **kw)
    if e.out_bf3:
        out = Bf3(torch.empty(B * Ho * Wo * Cout * 6, device=x3.data.device, dtype=torch.uint8), B * Ho * Wo, Cout)
    else:
        out = torch.empty((B, Ho, Wo, Cout), device=x3.data.device, dtype=torch.float32)
    check(_lib.load().a3r_conv3x3_bf3(x3.data_ptr(), wp3.data_ptr(), out.data_ptr(), B, H, W, Cin, Cout, stride, C.byref(e),
                                      stream_ptr()), "conv3x3_bf3")
    return out


def attention_bf3(q3: Bf3, k3: Bf3, v3: Bf3, B, H, Nq, Nk, q_col=0, k_col=0, v_col=0, out_pair=False) -> Bf3:
    """softmax(q k^T / 8) v per head (head_dim 64) on bf3 operands; q3/k3/v3 may be column slices (start column, multiple of 8)
    of wider bf3 matrices (e.g. the fused qkv projection).  Returns the bf3 [B*Nq, H*64] output."""
    o3 = Bf3(torch.zeros((B * Nq + (B * Nq & 1 if out_pair else 0)) * H * 64 * 6, device=q3.data.device, dtype=torch.uint8), B * Nq, H * 64,
             weight=bool(out_pair))
    check(_lib.load().a3r_attention_bf3(q3.data_ptr() + q_col * 6, q3.K, k3.data_ptr() + k_col * 6, k3.K, v3.data_ptr() + v_col * 6, v3.K,
                                        o3.data_ptr(), H * 64, B, H, Nq, Nk, int(out_pair), stream_ptr()), "attention_bf3")
    return o3


# ------------------------------------------------------------------------------------------------- fh2 (two fp16 planes)
class Fh2:
    """An fp32 matrix [rows, K] in fh2 form (two fp16 planes of scale * x, include/a3r.h): uint8 storage + shape + scale."""

    def __init__(self, data: torch.Tensor, rows: int, K: int, scale: float = 1.0):
        self.data, self.rows, self.K, self.scale = data, rows, K, float(scale)

    def data_ptr(self):
        return self.data.data_ptr()

    def planes(self):
        """-> float32 [2, rows, K]: the two planes (of scale * x)."""
        u = self.data.view(torch.float16).view(self.rows, self.K // 8, 2, 8)
        return u.permute(2, 0, 1, 3).reshape(2, self.rows, self.K).float()

    def value(self):
        """float64 [rows, K]: (h0 + h1) / scale."""
        p = self.planes().double()
        return (p[0] + p[1]) / self.scale


def fh2_weight_scale(w) -> float:
    """The power of two a3r_model_finalize would store these weights with (max|w| -> [2^12, 2^13))."""
    lib = _lib.load()
    out = torch.zeros(1, device=w.device, dtype=torch.float32)
    check(lib.a3r_absmax(ptr(_req(w, "w")), w.numel(), ptr(out), stream_ptr()), "absmax")
    return float(lib.a3r_fh2_weight_scale(float(out.item())))


def absmax_word(device):
    """A zeroed device word for the range statistics of an fh2 producer (max |stored value| as a float bit pattern)."""
    return torch.zeros(1, device=device, dtype=torch.int32)


def absmax_value(word) -> float:
    return float(word.view(torch.float32).item())


def split_fh2(x, scale=1.0, absmax=None) -> Fh2:
    """fp32 x [..., K] -> fh2 of scale * x (a3r_split_fh2); absmax: an absmax_word() receiving max |scale * x|."""
    _req(x, "x")
    K = x.shape[-1]
    M = x.numel() // K
    y = torch.empty(M * K * 4, device=x.device, dtype=torch.uint8)
    check(_lib.load().a3r_split_fh2(ptr(x), K, ptr(y), M, K, float(scale), ptr(absmax), stream_ptr()), "split_fh2")
    return Fh2(y, M, K, scale)


def split_fh2_w(w) -> Fh2:
    """Weights [N, K] -> fh2 with the automatic power-of-two scale."""
    return split_fh2(w, fh2_weight_scale(w))


def layernorm_fh2(x, w, b, eps=1e-6, scale=1.0, absmax=None) -> Fh2:
    _req(x, "x")
    D = x.shape[-1]
    M = x.numel() // D
    y = torch.empty(M * D * 4, device=x.device, dtype=torch.uint8)
    check(_lib.load().a3r_layernorm_fh2(ptr(x), ptr(_req(w, "w")), ptr(_req(b, "b")), ptr(y), M, D, eps, float(scale), ptr(absmax),
                                        stream_ptr()), "layernorm_fh2")
    return Fh2(y, M, D, scale)


def linear_fh2(x2: Fh2, w2: Fh2, bias=None, epi=_lib.EPI_NONE, out=None, **kw):
    """nn.Linear on the fp16 matrix cores with fp32-GEMM accuracy: x2 [M, K], w2 [N, K] in fh2 form with their own power-of-two
    scales (a3r_linear_fh2).  out_fh2=True returns an Fh2 (stored with out_scale), out_bf3=True a Bf3, otherwise fp32 [M, N]."""
    M, K, N = x2.rows, x2.K, w2.rows
    if w2.K != K:
        raise RuntimeError(f"linear_fh2: K mismatch ({K} vs {w2.K})")
    e = make_epilogue(epi, bias, x_scale=x2.scale, **kw)
    dev = x2.data.device
    if e.out_fh2:
        y = Fh2(torch.zeros(M * N * 4, device=dev, dtype=torch.uint8), M, N, e.out_scale or 1.0)
        check(_lib.load().a3r_linear_fh2(x2.data_ptr(), w2.data_ptr(), w2.scale, y.data_ptr(), N, M, N, K, C.byref(e), stream_ptr()), "linear_fh2")
        return y
    if e.out_bf3:
        y = Bf3(torch.zeros(M * N * 6, device=dev, dtype=torch.uint8), M, N)
        check(_lib.load().a3r_linear_fh2(x2.data_ptr(), w2.data_ptr(), w2.scale, y.data_ptr(), N, M, N, K, C.byref(e), stream_ptr()), "linear_fh2")
        return y
    if out is None:
        out = torch.empty((M, N), device=dev, dtype=torch.float32)
    check(_lib.load().a3r_linear_fh2(x2.data_ptr(), w2.data_ptr(), w2.scale, ptr(out), out.shape[-1], M, N, K, C.byref(e), stream_ptr()), "linear_fh2")
    return out


def linear_fh2_grouped(x2s, w2s, biases, epi=_lib.EPI_NONE, resids=None, out_scale=0.0, out_absmax=None, **kw):
    G = len(x2s)
    M, K, N = x2s[0].rows, x2s[0].K, w2s[0].rows
    outs = [torch.empty((M, N), device=x2s[0].data.device, dtype=torch.float32) for _ in range(G)]
    arr = (_lib.GroupPtrsFh2 * G)()
    for i in range(G):
        arr[i].x, arr[i].w, arr[i].y = x2s[i].data_ptr(), w2s[i].data_ptr(), outs[i].data_ptr()
        arr[i].bias = None if biases is None else biases[i].data_ptr()
        arr[i].resid = None if resids is None else resids[i].data_ptr()
        arr[i].w_scale = w2s[i].scale
        arr[i].x_scale = x2s[i].scale
        arr[i].out_scale = float(out_scale)
        arr[i].out_absmax = None if out_absmax is None else out_absmax.data_ptr()
    e = make_epilogue(epi, **kw)
    check(_lib.load().a3r_linear_fh2_grouped(arr, G, N, M, N, K, C.byref(e), stream_ptr()), "linear_fh2_grouped")
    return outs


def attention_fh2(q2: Fh2, k2: Fh2, v2: Fh2, B, H, Nq, Nk, q_col=0, k_col=0, v_col=0, out_scale=1.0, out_absmax=None) -> Fh2:
    """softmax(q k^T / 8) v per head (head_dim 64) on fh2 operands (a3r_attention_fh2); q2/k2/v2 may be column slices (start column,
    multiple of 8) of wider fh2 matrices, each stored with its own scale.  Returns the fh2 [B*Nq, H*64] output (stored with out_scale)."""
    o2 = Fh2(torch.zeros(B * Nq * H * 64 * 4, device=q2.data.device, dtype=torch.uint8), B * Nq, H * 64, out_scale)
    r = _lib.Fh2AttnRange(q2.scale, k2.scale, v2.scale, float(out_scale), None if out_absmax is None else out_absmax.data_ptr())
    check(_lib.load().a3r_attention_fh2(q2.data_ptr() + q_col * 4, q2.K, k2.data_ptr() + k_col * 4, k2.K, v2.data_ptr() + v_col * 4, v2.K,
                                        o2.data_ptr(), H * 64, B, H, Nq, Nk, C.byref(r), stream_ptr()), "attention_fh2")
    return o2


def attention_bf3_fh2out(q3: Bf3, k3: Bf3, v3: Bf3, B, H, Nq, Nk, q_col=0, k_col=0, v_col=0) -> Fh2:
    """attention_bf3 with the output written in fh2 form (the input of an fh2 output projection)."""
    o2 = Fh2(torch.zeros(B * Nq * H * 64 * 4, device=q3.data.device, dtype=torch.uint8), B * Nq, H * 64)
    check(_lib.load().a3r_attention_bf3_fh2out(q3.data_ptr() + q_col * 6, q3.K, k3.data_ptr() + k_col * 6, k3.K, v3.data_ptr() + v_col * 6,
                                               v3.K, o2.data_ptr(), H * 64, B, H, Nq, Nk, stream_ptr()), "attention_bf3_fh2out")
    return o2


def pack_conv3x3(w):
    Cout, Cin = w.shape[:2]
    wp = torch.empty((Cout, 3, 3, Cin), device=w.device, dtype=torch.float32)
    check(_lib.load().a3r_pack_conv3x3(ptr(_req(w, "w")), ptr(wp), Cout, Cin, stream_ptr()))
    return wp


def pack_convT(w):
    Cin, Cout, s, _ = w.shape
    wp = torch.empty((s * s * Cout, Cin), device=w.device, dtype=torch.float32)
    check(_lib.load().a3r_pack_convT(ptr(_req(w, "w")), ptr(wp), Cin, Cout, s, stream_ptr()))
    return wp


def conv3x3(x, wp, bias=None, stride=1, epi=_lib.EPI_NONE, **kw):
    """nn.Conv2d(k=3, padding=1, stride) on channels-last x [B,H,W,Cin] with packed weights [Cout,3,3,Cin]."""
    _req(x, "x"); _req(wp, "wp")
    B, H, W, Cin = x.shape
    Cout = wp.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((B, Ho, Wo, Cout), device=x.device, dtype=torch.float32)
    e = make_epilogue(epi, bias, **kw)
    check(_lib.load().a3r_conv3x3(ptr(x), ptr(wp), ptr(out), B, H, W, Cin, Cout, stride, C.byref(e), stream_ptr()), "conv3x3")
    return out


def conv_transpose(x, wpT, bias, s):
    """nn.ConvTranspose2d(kernel=stride=s) on channels-last x [B,H,W,Cin] with a3r_pack_convT weights."""
    B, H, W, Cin = x.shape
    Cout = wpT.shape[0] // (s * s)
    out = torch.empty((B, H * s, W * s, Cout), device=x.device, dtype=torch.float32)
    linear(x.reshape(B * H * W, Cin), wpT, bias, epi=_lib.EPI_PIXSHUF, out=out, pixshuf=(s, H, W, Cout))
    return out


def attention(q, k, v, H):
    """softmax(q k^T / 8) v for head_dim 64; q [B,Nq,H*64], k/v [B,Nk,H*64] (may be column slices of a wider buffer)."""
    B, Nq, _ = q.shape
    Nk = k.shape[1]
    for t in (q, k, v):
        if t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
            raise RuntimeError("attention operands must be row-strided views [B, N, ld]")
    o = torch.empty((B, Nq, H * 64), device=q.device, dtype=torch.float32)
    check(_lib.load().a3r_attention(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(o), H * 64, B, H, Nq, Nk,
                                    stream_ptr()), "attention")
    return o


def patchify(img, channels_last=False):
    """im2col of the 16x16/stride-16 patch embedding; img [B,3,H,W] (or [B,H,W,3] if channels_last)."""
    _req(img, "img")
    if channels_last:
        B, H, W, Cc = img.shape
        strides = (H * W * Cc, 1, W * Cc, Cc)
    else:
        B, Cc, H, W = img.shape
        strides = (Cc * H * W, H * W, W, 1)
    cols = torch.empty((B * (H // 16) * (W // 16), Cc * 256), device=img.device, dtype=torch.float32)
    check(_lib.load().a3r_patchify(ptr(img), ptr(cols), B, Cc, H, W, *strides, stream_ptr()), "patchify")
    return cols


def conv3x3_fh2(x2: Fh2, wp2: Fh2, shape, bias=None, stride=1, epi=_lib.EPI_NONE, **kw):
    """3x3 conv (padding 1) on the fh2 kernel: x2 = fh2 of the channels-last map `shape` = (B, H, W, Cin), wp2 = fh2 of the packed
    weights [Cout, 9 Cin] (split_fh2_w).  Returns fp32 [B, Ho, Wo, Cout] (or an Fh2 with out_fh2=True); aux_fh2=Fh2 also receives
    the fh2 form of the result (through a ReLU with aux_relu=True)."""
    B, H, W, Cin = shape
    Cout = wp2.rows
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    e = make_epilogue(epi, bias, x_scale=x2.scale, **kw)
    dev = x2.data.device
    if e.out_fh2:
        out = Fh2(torch.zeros(B * Ho * Wo * Cout * 4, device=dev, dtype=torch.uint8), B * Ho * Wo, Cout, e.out_scale or 1.0)
    elif epi == _lib.EPI_HEAD:
        out = torch.empty((B, Ho, Wo, 3), device=dev, dtype=torch.float32)          # pts3d; conf goes to head[2]
    else:
        out = torch.empty((B, Ho, Wo, Cout), device=dev, dtype=torch.float32)
    check(_lib.load().a3r_conv3x3_fh2(x2.data_ptr(), wp2.data_ptr(), wp2.scale, out.data_ptr(), B, H, W, Cin, Cout, stride, C.byref(e),
                                      stream_ptr()), "conv3x3_fh2")
    return out


def upsample2x_fh2(x, crop=None, scale=1.0, absmax=None) -> Fh2:
    """upsample2x written in fh2 form (rows = output pixels, K = C), stored with `scale`."""
    _req(x, "x")
    B, H, W, Cc = x.shape
    Hc, Wc = crop if crop else (2 * H, 2 * W)
    out = Fh2(torch.zeros(B * Hc * Wc * Cc * 4, device=x.device, dtype=torch.uint8), B * Hc * Wc, Cc, scale)
    check(_lib.load().a3r_upsample2x_fh2(ptr(x), out.data_ptr(), B, H, W, Cc, Hc, Wc, float(scale), ptr(absmax), stream_ptr()), "upsample2x_fh2")
    return out


def upsample2x_bf3(x, crop=None) -> Bf3:
    """upsample2x written in bf3 form (rows = output pixels, K = C; a3r_upsample2x_bf3)."""
    _req(x, "x")
    B, H, W, Cc = x.shape
    Hc, Wc = crop if crop else (2 * H, 2 * W)
    out = Bf3(torch.zeros(B * Hc * Wc * Cc * 6, device=x.device, dtype=torch.uint8), B * Hc * Wc, Cc)
    check(_lib.load().a3r_upsample2x_bf3(ptr(x), out.data_ptr(), B, H, W, Cc, Hc, Wc, stream_ptr()), "upsample2x_bf3")
    return out


def upsample2x(x, crop=None):
    """F.interpolate(scale_factor=2, bilinear, align_corners=True) on channels-last [B,H,W,C]."""
    _req(x, "x")
    B, H, W, Cc = x.shape
    Hc, Wc = crop if crop else (2 * H, 2 * W)
    out = torch.empty((B, Hc, Wc, Cc), device=x.device, dtype=torch.float32)
    check(_lib.load().a3r_upsample2x(ptr(x), ptr(out), B, H, W, Cc, Hc, Wc, stream_ptr()), "upsample2x")
    return out


def head_final(x, w, b):
    """conv1x1 (C -> 4) + postprocess (postprocess.py:10-58) on channels-last x [..., C]."""
    _req(x, "x")
    Cc = x.shape[-1]
    P = x.numel() // Cc
    pts = torch.empty(x.shape[:-1] + (3,), device=x.device, dtype=torch.float32)
    conf = torch.empty(x.shape[:-1], device=x.device, dtype=torch.float32)
    check(_lib.load().a3r_head_final(ptr(x), ptr(_req(w.reshape(4, Cc), "w")), ptr(_req(b, "b")), ptr(pts), ptr(conf), P, Cc,
                                     stream_ptr()), "head_final")
    return pts, conf


# ---- the flow network's kernels without a GEMM shape (csrc/raft.hip, a3r_flow_*), through the launchers the network's plan uses
def _flow_out(out, shape, like, name):
    if out is None:
        return torch.empty(shape, device=like.device, dtype=torch.float32)
    if tuple(_req(out, name).shape) != tuple(shape):
        raise RuntimeError(f"{name} must have shape {tuple(shape)}")
    return out


def flow_conv7_planes(x0, w, bias=None, x1=None, in_mul=1.0, in_add=0.0, relu=True, form=0, out=None):
    """7x7 convolution, padding 3, stride 2, of the planes x0 [B, c, H, W] (x1: a second source, concatenated along channels), every
    element entering as x * in_mul + in_add; w [Cout, Cin, 7, 7] -> channels-last [B, Ho, Wo, Cout].  form 1: the generic kernel."""
    B, c, H, W = _req(x0, "x0").shape
    if x1 is not None and _req(x1, "x1").shape != x0.shape:
        raise RuntimeError("x1 must have the shape of x0")
    Cout, Cin = w.shape[:2]
    if tuple(_req(w, "w").shape) != (Cout, c * (2 if x1 is not None else 1), 7, 7):
        raise RuntimeError("w must be [Cout, Cin, 7, 7] with Cin the channels of the sources")
    if bias is not None and tuple(_req(bias, "bias").shape) != (Cout,):
        raise RuntimeError("bias must be [Cout]")
    out = _flow_out(out, (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout), x0, "out")
    wt = torch.empty(Cin * 49 * Cout, device=x0.device, dtype=torch.float32)
    check(_lib.load().a3r_flow_conv7_planes(ptr(x0), ptr(x1), c, ptr(w), ptr(bias), ptr(wt), ptr(out), B, H, W, Cout, in_mul, in_add,
                                            int(relu), form, stream_ptr()), "flow_conv7_planes")
    return out


def flow_conv7_flow(flow, w, bias=None, relu=True, form=0, out=None):
    """7x7 convolution, padding 3, stride 1, of the channels-last coarse flow [B, h, w, 2]; w [Cout, 2, 7, 7] -> [B, h, w, Cout]."""
    B, h, wd, two = _req(flow, "flow").shape
    Cout = w.shape[0]
    if two != 2 or tuple(_req(w, "w").shape) != (Cout, 2, 7, 7):
        raise RuntimeError("flow must be [B, h, w, 2] and w [Cout, 2, 7, 7]")
    if bias is not None and tuple(_req(bias, "bias").shape) != (Cout,):
        raise RuntimeError("bias must be [Cout]")
    out = _flow_out(out, (B, h, wd, Cout), flow, "out")
    wt = torch.empty(98 * Cout, device=flow.device, dtype=torch.float32)
    check(_lib.load().a3r_flow_conv7_flow(ptr(flow), ptr(w), ptr(bias), ptr(wt), ptr(out), B, h, wd, Cout, int(relu), form, stream_ptr()),
          "flow_conv7_flow")
    return out


def flow_dwconv7(x, w, bias, out=None):
    """depthwise 7x7, padding 3, on channels-last x [B, h, w, C]; w [C, 1, 7, 7] or [C, 49], bias [C]."""
    B, h, wd, Cc = _req(x, "x").shape
    if _req(w, "w").numel() != Cc * 49 or w.shape[0] != Cc or tuple(_req(bias, "bias").shape) != (Cc,):
        raise RuntimeError("w must be [C, 49] and bias [C]")
    out = _flow_out(out, x.shape, x, "out")
    wt = torch.empty(49 * Cc, device=x.device, dtype=torch.float32)
    check(_lib.load().a3r_flow_dwconv7(ptr(x), ptr(w), ptr(bias), ptr(wt), ptr(out), B, h, wd, Cc, stream_ptr()), "flow_dwconv7")
    return out


def flow_gather_s2(x, out=None):
    """x [B, h, w, C][:, ::2, ::2] (the sampling of a 1x1 convolution with stride 2); C % 4 == 0."""
    B, h, wd, Cc = _req(x, "x").shape
    out = _flow_out(out, (B, (h - 1) // 2 + 1, (wd - 1) // 2 + 1, Cc), x, "out")
    check(_lib.load().a3r_flow_gather_s2(ptr(x), ptr(out), B, h, wd, Cc, stream_ptr()), "flow_gather_s2")
    return out


def flow_halve(x, out=None):
    """F.interpolate(scale_factor=0.5, mode='bilinear') of channels-last x [B, h, w, C]: 2x2 means -> [B, h // 2, w // 2, C]."""
    B, h, wd, Cc = _req(x, "x").shape
    out = _flow_out(out, (B, h // 2, wd // 2, Cc), x, "out")
    check(_lib.load().a3r_flow_halve(ptr(x), ptr(out), B, h, wd, Cc, stream_ptr()), "flow_halve")
    return out


def flow_corr_lookup(corr, flow, r, ldo=None, out=None):
    """Correlation lookup: corr, a list of levels [B h w, h_l, w_l]; flow [B, h, w, 2] -> [B h w, ldo], channel l (2r+1)^2 + a (2r+1) + c,
    the columns past levels (2r+1)^2 zero."""
    B, h, wd, two = _req(flow, "flow").shape
    n = len(corr)
    if two != 2 or not 1 <= n <= 4 or any(_req(c, "corr").dim() != 3 or c.shape[0] != B * h * wd for c in corr):
        raise RuntimeError("flow must be [B, h, w, 2] and corr 1..4 levels [B h w, h_l, w_l]")
    ldo = n * (2 * r + 1) ** 2 if ldo is None else ldo
    out = _flow_out(out, (B * h * wd, ldo), flow, "out")
    ptrs = (C.c_void_p * n)(*[c.data_ptr() for c in corr])
    hl, wl = (C.c_int * n)(*[c.shape[1] for c in corr]), (C.c_int * n)(*[c.shape[2] for c in corr])
    check(_lib.load().a3r_flow_corr_lookup(ptrs, hl, wl, ptr(flow), ptr(out), ldo, B, h, wd, r, n, stream_ptr()), "flow_corr_lookup")
    return out


def flow_convex_upsample(flow, mask, out=None):
    """Convex up-sampling: flow [B, h, w, 2], mask [B, h, w, 576] (channel k 64 + i 8 + j) -> [B, 2, 8 h, 8 w]."""
    B, h, wd, two = _req(flow, "flow").shape
    if two != 2 or tuple(_req(mask, "mask").shape) != (B, h, wd, 576):
        raise RuntimeError("flow must be [B, h, w, 2] and mask [B, h, w, 576]")
    out = _flow_out(out, (B, 2, 8 * h, 8 * wd), flow, "out")
    check(_lib.load().a3r_flow_convex_upsample(ptr(flow), ptr(mask), ptr(out), B, h, wd, stream_ptr()), "flow_convex_upsample")
    return out


def flow_scale(x, s):
    """x *= s, in place."""
    check(_lib.load().a3r_flow_scale(ptr(_req(x, "x")), s, x.numel(), stream_ptr()), "flow_scale")
    return x


def flow_pack_cols(dst, c0, src, Cs=None):
    """dst [rows, ldd][:, c0:c0 + Cs] = src [rows, lds][:, :Cs], in place."""
    rows, ldd = _req(dst, "dst").shape
    if _req(src, "src").dim() != 2 or src.shape[0] != rows:
        raise RuntimeError("src must have the rows of dst")
    Cs = src.shape[1] if Cs is None else Cs
    check(_lib.load().a3r_flow_pack_cols(ptr(dst), ldd, c0, ptr(src), src.shape[1], Cs, rows, stream_ptr()), "flow_pack_cols")
    return dst


def flow_add(flow, upd):
    """flow [rows, 2] += upd [rows, ldu][:, :2], in place."""
    rows, two = _req(flow, "flow").shape
    if two != 2 or _req(upd, "upd").dim() != 2 or upd.shape[0] != rows:
        raise RuntimeError("flow must be [rows, 2] and upd [rows, ldu]")
    check(_lib.load().a3r_flow_add(ptr(flow), ptr(upd), upd.shape[1], rows, stream_ptr()), "flow_add")
    return flow


def flow_image_absmax(x):
    """max |x| of every image of x [images, ...] -> float32 [images] (the bits of a non-negative float, as the kernel's atomic max leaves them)."""
    images = _req(x, "x").shape[0]
    out = torch.full((images,), -1, device=x.device, dtype=torch.int32)
    check(_lib.load().a3r_flow_image_absmax(ptr(x), x.numel() // images, images, ptr(out), stream_ptr()), "flow_image_absmax")
    return out.view(torch.float32)


MOTION_ENTRY = np.dtype([('depth_row', '<i4'), ('flow_row', '<i4'), ('image', '<i4'), ('pad', '<i4'), ('depth_rt', '<f4', (4,)),
                         ('Hm', '<f4', (9,)), ('Kt', '<f4', (3,))])


def motion_masks(pred_i, pred_j, flow_ij, flow_ji, entries, lists, thre, want_mean=False):
    """Self-computed motion masks from prepared pair geometry (cloud_opt_flow/optimizer.py:201-235; a3r_motion_masks, csrc/motion.hip).
    pred_i, pred_j [E,P,3] (or [E,H,W,3]) and flow_ij, flow_ji [E,2,H,W]: contiguous float32 device tensors.  entries: numpy array of
    MOTION_ENTRY, one record per directed entry (2M of them).  lists: per image the entry indices whose normalised errors are
    averaged, in that order.  Returns masks [N,H,W] bool (device), and the mean normalised error [N,H,W] with want_mean."""
    lib = _lib.load()
    for t, name in ((pred_i, "pred_i"), (pred_j, "pred_j"), (flow_ij, "flow_ij"), (flow_ji, "flow_ji")):
        _req(t, name)
    E, _, H, W = flow_ij.shape
    P, N = H * W, len(lists)
    if not (flow_ji.shape == flow_ij.shape and pred_i.numel() == pred_j.numel() == E * P * 3):
        raise RuntimeError("motion_masks: pred_i / pred_j [E,P,3] and flow_ij / flow_ji [E,2,H,W] do not agree")
    entries = np.ascontiguousarray(entries, dtype=MOTION_ENTRY)
    assert MOTION_ENTRY.itemsize == C.sizeof(_lib.MotionEntry)
    if len(entries) % 2 or not len(entries):
        raise RuntimeError("motion_masks: the entry table holds two records per symmetric pair")
    M = len(entries) // 2
    start = np.zeros(N + 1, np.int32)
    start[1:] = np.cumsum([len(l) for l in lists])
    flat = np.ascontiguousarray([k for l in lists for k in l], dtype=np.int32)
    dev = pred_i.device
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)
    entries_dev, start_dev, flat_dev = up(entries), up(start), up(flat)
    ws_bytes = int(lib.a3r_motion_workspace_bytes(M, N, P))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    masks = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    mean = torch.empty((N, H, W), dtype=torch.float32, device=dev) if want_mean else None
    d = _lib.MotionDesc(M, N, E, H, W, float(thre), ptr(pred_i), ptr(pred_j), ptr(flow_ij), ptr(flow_ji), ptr(entries_dev),
                        entries.ctypes.data, ptr(start_dev), start.ctypes.data, ptr(flat_dev), flat.ctypes.data if len(flat) else None)
    with torch.cuda.device(dev):
        check(lib.a3r_motion_masks(C.byref(d), ptr(ws), ws_bytes, ptr(masks), ptr(mean), stream_ptr()), "a3r_motion_masks")
    masks = masks.bool()          # stream-ordered after the kernels; the uploaded tables and the workspace are freed stream-ordered too
    return (masks, mean) if want_mean else masks


class PrepTables:
    """The resample tables of one (source size, resized size, filter) on one device (a3r_prep_desc, csrc/prep.hip): per axis
    [new_len, taps] clipped source indices and float64 weights, exactly what image_pose.resize_tables returns, kept on the host (int32:
    validated there by the C call) and on the device.  x_tab = (idx, w) of the width axis [Wr, taps], y_tab of the height axis."""

    def __init__(self, x_tab, y_tab, device):
        self.device = torch.device(device)
        (ix, wx), (iy, wy) = x_tab, y_tab
        self.idx_x, self.idx_y = (np.ascontiguousarray(a, dtype=np.int32) for a in (ix, iy))
        self.w_x, self.w_y = (np.ascontiguousarray(a, dtype=np.float64) for a in (wx, wy))
        if not (self.idx_x.ndim == 2 and self.idx_x.shape == self.w_x.shape and self.idx_y.shape == self.w_y.shape and
                self.idx_x.shape[1] == self.idx_y.shape[1]):
            raise RuntimeError("PrepTables: idx and w of an axis are [new_len, taps], with one taps for both axes")
        if not (np.array_equal(self.idx_x, ix) and np.array_equal(self.idx_y, iy)):
            raise RuntimeError("PrepTables: an index does not fit int32")
        self.Wr, self.taps = self.idx_x.shape
        self.Hr = self.idx_y.shape[0]
        up = lambda a: torch.from_numpy(a).to(self.device)
        self.idx_x_dev, self.w_x_dev, self.idx_y_dev, self.w_y_dev = up(self.idx_x), up(self.w_x), up(self.idx_y), up(self.w_y)
        self.device = self.idx_x_dev.device                        # with its index: 'cuda' has become 'cuda:0'

    def desc(self, Hs, Ws, crop):
        y0, x0, Hc, Wc = (int(c) for c in crop)
        return _lib.PrepDesc(Hs, Ws, self.Hr, self.Wr, self.taps, y0, x0, Hc, Wc, ptr(self.idx_x_dev), self.idx_x.ctypes.data,
                             ptr(self.w_x_dev), ptr(self.idx_y_dev), self.idx_y.ctypes.data, ptr(self.w_y_dev))


def _prep_resample(call, what, src, Hs, Ws, tables, crop, *lead):
    lib = _lib.load()
    if not isinstance(tables, PrepTables):
        tables = PrepTables(tables[0], tables[1], src.device)
    if tables.device != src.device:
        raise RuntimeError(f"{what}: the tables are on {tables.device}, the source on {src.device}")
    crop = (0, 0, tables.Hr, tables.Wr) if crop is None else crop
    d = tables.desc(Hs, Ws, crop)
    ws_bytes = int(lib.a3r_prep_workspace_bytes(Hs, Ws, d.Wc))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=src.device)
    out = torch.empty((max(d.Hc, 0), max(d.Wc, 0), 3), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        check(getattr(lib, call)(ptr(src), *lead, C.byref(d), ptr(ws), ws_bytes, ptr(out), stream_ptr()), what)
    return out            # the workspace is freed stream-ordered after the kernels


def prep_pointmap(depth, focal, tables, crop=None):
    """crop_center(resize(pixel_to_pointcloud(depth, focal))) of dust3r/utils/image_pose.py on the device, the same numbers
    (a3r_prep_pointmap, csrc/prep.hip).  depth [Hs, Ws]: contiguous float32 device tensor.  focal: anything float() takes (a float32
    0-d array, the integer 200).  tables: a PrepTables, or ((idx_x, w_x), (idx_y, w_y)) from image_pose.resize_tables.
    crop = (y0, x0, Hc, Wc): the window of the resized map (default: all of it).  Returns [Hc, Wc, 3] float32 on depth's device."""
    _req(depth, "depth")
    if depth.dim() != 2:
        raise RuntimeError("prep_pointmap: depth is [Hs, Ws]")
    return _prep_resample("a3r_prep_pointmap", "prep_pointmap", depth, depth.shape[0], depth.shape[1], tables, crop, float(focal))


def prep_resize3(src, tables, crop=None):
    """cv2_resize of image_pose.py (then crop_center) on a float32 [Hs, Ws, 3] device tensor with the host's tables (a3r_prep_resize3)."""
    _req(src, "src")
    if src.dim() != 3 or src.shape[2] != 3:
        raise RuntimeError("prep_resize3: src is [Hs, Ws, 3]")
    return _prep_resample("a3r_prep_resize3", "prep_resize3", src, src.shape[0], src.shape[1], tables, crop)


def prep_image(u8):
    """ImgNorm and the validity mask of load_images on the device (a3r_prep_image).  u8 [H, W, 3]: contiguous uint8 device tensor (the PIL
    image after resize and crop).  Returns img [3, H, W] float32 = (u / 255 - 0.5) / 0.5 and mask [H, W] bool = ~(sum_c u_c / 255 <= 0.01)."""
    if not (isinstance(u8, torch.Tensor) and u8.is_cuda and u8.dtype == torch.uint8 and u8.is_contiguous() and u8.dim() == 3 and u8.shape[2] == 3):
        raise RuntimeError("prep_image: u8 must be a contiguous uint8 CUDA tensor [H, W, 3]")
    H, W = u8.shape[:2]
    img = torch.empty((3, H, W), dtype=torch.float32, device=u8.device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=u8.device)
    with torch.cuda.device(u8.device):
        check(_lib.load().a3r_prep_image(ptr(u8), H, W, ptr(img), ptr(mask), stream_ptr()), "prep_image")
    return img, mask.view(torch.bool)


def _depth_eval_args(pred, gt, what):
    for t, name in ((pred, "pred"), (gt, "gt")):
        _req(t, name)
    if pred.shape != gt.shape:
        raise ValueError(f"{what}: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    if pred.device != gt.device:
        raise RuntimeError(f"{what}: pred is on {pred.device}, gt on {gt.device}")
    lib = _lib.load()
    n = pred.numel()
    ws_bytes = int(lib.a3r_depth_eval_workspace_bytes(n))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=pred.device)
    return lib, n, ws, ws_bytes


def depth_align(pred, gt, depth_max=70.0, mode="lad"):
    """One scale and shift for the whole clip over the pixels with 1e-3 < gt < depth_max (a3r_depth_align, csrc/metrics.hip; the rules
    of tool/depth_metrics.align_depth).  pred, gt: contiguous float32 device tensors of one shape.  mode: 'lad', 'lstsq', 'scale',
    'median'.  Enqueue-only; returns device tensors st [2] float64 = (scale, shift) and info [16] float64 (include/a3r.h: n_valid, the
    LAD objective, passes, enlargements, the middle order statistics of pred and of gt, the medians, the LAD normalisation)."""
    if mode not in _lib.DEPTH_ALIGN_MODES:
        raise ValueError(f"bad alignment {mode=}")
    lib, n, ws, ws_bytes = _depth_eval_args(pred, gt, "depth_align")
    st = torch.empty(2, dtype=torch.float64, device=pred.device)
    info = torch.empty(_lib.DEPTH_INFO_DOUBLES, dtype=torch.float64, device=pred.device)
    with torch.cuda.device(pred.device):
        check(lib.a3r_depth_align(ptr(pred), ptr(gt), n, float(depth_max), _lib.DEPTH_ALIGN_MODES[mode], ptr(ws), ws_bytes, ptr(st), ptr(info),
                                  stream_ptr()), "depth_align")
    return st, info           # the workspace is freed stream-ordered after the kernels


def depth_metrics(pred, gt, depth_max, scale, shift=None):
    """AbsRel, SqRel, RMSE, logRMSE, delta < 1.25^k, n_valid of clip(scale * pred + shift, 1e-5, depth_max) against gt over the pixels
    with 1e-3 < gt < depth_max (a3r_depth_metrics).  scale, shift: two numbers, or scale = the device tensor [2] float64 that depth_align
    returned (then nothing leaves the device in between).  Enqueue-only; returns a device tensor [8] float64 in that order."""
    lib, n, ws, ws_bytes = _depth_eval_args(pred, gt, "depth_metrics")
    if isinstance(scale, torch.Tensor) and shift is None:
        st = scale
        if not (st.is_cuda and st.device == pred.device and st.dtype == torch.float64 and st.is_contiguous() and st.numel() == 2):
            raise RuntimeError("depth_metrics: (scale, shift) as a tensor must be a contiguous float64 tensor [2] on pred's device")
    else:
        st = torch.tensor([float(scale), float(shift)], dtype=torch.float64).to(pred.device)
    out = torch.empty(_lib.DEPTH_METRIC_DOUBLES, dtype=torch.float64, device=pred.device)
    with torch.cuda.device(pred.device):
        check(lib.a3r_depth_metrics(ptr(pred), ptr(gt), n, float(depth_max), ptr(st), ptr(ws), ws_bytes, ptr(out), stream_ptr()), "depth_metrics")
    return out


def _req_points(t, name):
    _req(t, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{name} must be [n, 3]")
    return t


def nn_chunks(n_query, n_data, chunks=0) -> int:
    """The number of data ranges a search of these sizes uses (a3r_nn_chunks): `chunks` itself when forced, the library's choice for 0."""
    return int(_lib.load().a3r_nn_chunks(int(n_query), int(n_data), int(chunks)))


def nn_search(query, data, chunks=0, return_dist=False):
    """Exact nearest neighbour of every query point among the data points (a3r_nn_search, csrc/match.hip): float64 squared distances
    from direct differences, the lowest index of a tie, -1 where no data point is at a finite distance (include/a3r.h has the
    definition).  query [nq,3], data [nd,3]: contiguous float32 device tensors.  chunks: 0 = the library's choice, >= 1 forces that
    many data ranges (the result does not depend on it).  Enqueue-only; returns index [nq] int32, and with return_dist also the
    squared distance [nq] float64 (+inf where the index is -1)."""
    _req_points(query, "query"); _req_points(data, "data")
    if query.device != data.device:
        raise RuntimeError(f"nn_search: query is on {query.device}, data on {data.device}")
    lib, dev = _lib.load(), query.device
    nq, nd = query.shape[0], data.shape[0]
    ws_bytes = int(lib.a3r_nn_workspace_bytes(nq, nd, int(chunks)))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    index = torch.empty(nq, dtype=torch.int32, device=dev)
    dist = torch.empty(nq, dtype=torch.float64, device=dev) if return_dist else None
    with torch.cuda.device(dev):
        check(lib.a3r_nn_search(ptr(query), nq, ptr(data), nd, int(chunks), ptr(ws), ws_bytes, ptr(index), ptr(dist), stream_ptr()), "nn_search")
    return (index, dist) if return_dist else index          # the workspace is freed stream-ordered after the kernels


def reciprocal_matches(p1, p2, chunks=0):
    """find_reciprocal_matches (dust3r/utils/geometry.py:351-367) on the device with nn_search's neighbour rule (a3r_reciprocal_matches).
    p1 [n1,3], p2 [n2,3]: contiguous float32 device tensors.  Returns a dict of device tensors: nn2_in_P1 [n2] int32, nn1_in_P2 [n1]
    int32, reciprocal_in_P2 [n2] bool, pairs [M,2] int32 = (k1, k2) of the reciprocal k2 in ascending k2, and count = M (an int: the
    call synchronises once to learn it)."""
    _req_points(p1, "p1"); _req_points(p2, "p2")
    if p1.device != p2.device:
        raise RuntimeError(f"reciprocal_matches: p1 is on {p1.device}, p2 on {p2.device}")
    lib, dev = _lib.load(), p1.device
    n1, n2 = p1.shape[0], p2.shape[0]
    ws_bytes = int(lib.a3r_match_workspace_bytes(n1, n2, int(chunks)))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    nn2 = torch.empty(n2, dtype=torch.int32, device=dev)
    nn1 = torch.empty(n1, dtype=torch.int32, device=dev)
    rec = torch.empty(n2, dtype=torch.uint8, device=dev)
    cap = min(n1, n2)                                        # a k1 is the partner of at most one k2
    pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    count = C.c_longlong(0)
    with torch.cuda.device(dev):
        check(lib.a3r_reciprocal_matches(ptr(p1), n1, ptr(p2), n2, int(chunks), ptr(ws), ws_bytes, ptr(nn2), ptr(nn1), ptr(rec), cap,
                                         ptr(pairs), C.byref(count), stream_ptr()), "reciprocal_matches")
    M = int(count.value)
    return dict(nn2_in_P1=nn2, nn1_in_P2=nn1, reciprocal_in_P2=rec.view(torch.bool), pairs=pairs[:M], count=M)


def render_set_form(form: int) -> int:
    """The splat's form (a3r_render_set_form; bit 0: a grid axis over the cameras, bit 1: no read before the atomic, bit 2: the reads
    one pixel at a time): a developer's A/B switch that does not change the pictures.  Returns the previous value; -1 only queries."""
    return int(_lib.load().a3r_render_set_form(int(form)))


def _host_f64(a, name):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.dtype != np.float64:
        raise ValueError(f"render_points: {name} must be float64, got {a.dtype}")
    return a


def render_cameras(w2c, K):
    """The camera table of render_points, [C,16] float64 (a3r_render_cam: [R|t] row-major, fx, fy, cx, cy), from w2c [C,3,4] or
    [C,4,4] and K [C,3,3], both float64 (numpy or torch).  A non-zero skew is a ValueError."""
    w2c, K = _host_f64(w2c, "w2c"), _host_f64(K, "K")
    if w2c.ndim != 3 or w2c.shape[1] not in (3, 4) or w2c.shape[2] != 4:
        raise ValueError(f"render_points: w2c is [C,3,4] or [C,4,4], got {w2c.shape}")
    C_ = w2c.shape[0]
    if K.shape != (C_, 3, 3):
        raise ValueError(f"render_points: K is [C,3,3] with C = {C_}, got {K.shape}")
    if np.any(K[:, 0, 1] != 0):
        raise ValueError("render_points: K has a non-zero skew K[0,1]; the renderer's cameras are fx, fy, cx, cy")
    cams = np.empty((C_, 16), np.float64)
    cams[:, :12] = w2c[:, :3, :].reshape(C_, 12)
    cams[:, 12], cams[:, 13], cams[:, 14], cams[:, 15] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    return cams


def render_points(xyz, rgb=None, w2c=None, K=None, shape=None, radius=0, near=1e-6, background=(255, 255, 255), want_index=False,
                  cams=None):
    """A point cloud drawn into the pictures of C pinhole cameras as z-buffered square splats (a3r_render_points, csrc/render.hip;
    include/a3r.h has the definition: float64 projection, half-to-even pixel, the nearest point wins a pixel and the lowest index an
    exact depth tie -- bitwise reproducible).  xyz [M,3]: contiguous float32 device tensor; rgb [M,3]: contiguous uint8 device
    tensor or None.  w2c [C,3,4] or [C,4,4] and K [C,3,3]: float64 world-to-camera transforms and intrinsics (tool/render.py:
    world_to_camera inverts poses), or cams = the table render_cameras() made of them.  shape = (H, W); radius in [0, 8]: the
    splat covers (2 radius + 1)^2 pixels; near: the smallest camera depth that draws.  Enqueue-only; returns a dict of device
    tensors: depth [C,H,W] float32 (0 where nothing landed), rgb [C,H,W,3] uint8 (with rgb; `background` where nothing landed) and,
    with want_index, index [C,H,W] int32 (the winner's row of xyz, -1 where nothing landed)."""
    _req_points(xyz, "xyz")
    if rgb is not None and not (isinstance(rgb, torch.Tensor) and rgb.device == xyz.device and rgb.dtype == torch.uint8 and rgb.is_contiguous()
                                and rgb.shape == xyz.shape):
        raise RuntimeError("render_points: rgb must be a contiguous uint8 tensor [M,3] on xyz's device")
    if cams is None:
        if w2c is None or K is None:
            raise ValueError("render_points: w2c and K (or cams) are needed")
        cams = render_cameras(w2c, K)
    cams = np.ascontiguousarray(cams, dtype=np.float64)
    if cams.ndim != 2 or cams.shape[1] != 16:
        raise ValueError(f"render_points: cams is [C,16], got {cams.shape}")
    if shape is None or len(shape) != 2:
        raise ValueError("render_points: shape = (H, W) is needed")
    H, W = int(shape[0]), int(shape[1])
    bg = np.asarray(background)
    if bg.shape != (3,) or np.any(bg != bg.astype(np.uint8)):
        raise ValueError(f"render_points: background is three values in [0, 255], got {background!r}")
    bg = np.ascontiguousarray(bg, dtype=np.uint8)
    assert C.sizeof(_lib.RenderCam) == 128 == cams.strides[0]
    lib, dev, n_cams, M = _lib.load(), xyz.device, cams.shape[0], xyz.shape[0]
    ws_bytes = int(lib.a3r_render_workspace_bytes(n_cams, H, W))            # 0 for sizes the call below refuses
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    out_shape = (n_cams, H, W) if ws_bytes else (0, 0, 0)
    depth = torch.empty(out_shape, dtype=torch.float32, device=dev)
    out_rgb = torch.empty(out_shape + (3,), dtype=torch.uint8, device=dev) if rgb is not None else None
    index = torch.empty(out_shape, dtype=torch.int32, device=dev) if want_index else None
    cams_dev = torch.from_numpy(cams.reshape(-1).copy()).to(dev) if n_cams else None
    with torch.cuda.device(dev):
        check(lib.a3r_render_points(ptr(xyz), ptr(rgb), M, ptr(cams_dev), cams.ctypes.data if n_cams else None, n_cams, H, W, int(radius),
                                    float(near), bg.ctypes.data, ptr(ws), ws_bytes, ptr(depth), ptr(out_rgb), ptr(index), stream_ptr()),
              "render_points")
    out = dict(depth=depth)              # the camera table and the workspace are freed stream-ordered after the kernels
    if out_rgb is not None:
        out["rgb"] = out_rgb
    if index is not None:
        out["index"] = index
    return out


VOXEL_REDUCE = {"best": _lib.VOXEL_BEST, "mean": _lib.VOXEL_MEAN}


def voxel_default_slots(M: int) -> int:
    """The table size voxel_downsample(slots=0) uses: the smallest power of two >= 2 M, at most 2^31."""
    s = 1
    while s < 2 * M and s < (1 << 31):
        s <<= 1
    return s


def _voxel_args(xyz, voxel, priority, rgb, reduce, min_count, slots):
    """The checks of voxel_downsample; every refusal is a ValueError raised before the library is touched.  The scalars first, then
    every tensor's type, dtype, shape and layout, the devices last."""
    voxel = float(voxel)
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError(f"voxel_downsample: voxel = {voxel} must be finite and positive")
    if reduce not in VOXEL_REDUCE:
        raise ValueError(f"voxel_downsample: reduce = {reduce!r} is neither 'best' nor 'mean'")
    if int(min_count) != min_count or min_count < 1:
        raise ValueError(f"voxel_downsample: min_count = {min_count!r} must be an integer >= 1")
    if int(slots) != slots or slots < 0 or int(slots) & (int(slots) - 1):
        raise ValueError(f"voxel_downsample: slots = {slots!r} must be 0 or a power of two above the point count")
    slots = int(slots)

    def tensor(t, name, dtype, shape):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"voxel_downsample: {name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != dtype:
            raise ValueError(f"voxel_downsample: {name} must be {dtype}, got {t.dtype}")
        if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
            raise ValueError(f"voxel_downsample: {name} has shape {tuple(t.shape)}, expected {['M' if w is None else w for w in shape]}")
        if not t.is_contiguous():
            raise ValueError(f"voxel_downsample: {name} must be contiguous")
    tensor(xyz, "xyz", torch.float32, (None, 3))
    M = xyz.shape[0]
    if priority is not None:
        tensor(priority, "priority", torch.float32, (M,))
    if rgb is not None:
        tensor(rgb, "rgb", torch.uint8, (M, 3))
    if M >= 1 << 31:
        raise ValueError(f"voxel_downsample: M = {M} points: the count must stay below 2^31")
    if slots and (slots <= M or slots > 1 << 31):
        raise ValueError(f"voxel_downsample: slots = {slots} must exceed the {M} points and stay at or below 2^31")
    for t, name in ((xyz, "xyz"), (priority, "priority"), (rgb, "rgb")):
        if t is not None and (t.device.type != "cuda" or t.device != xyz.device):
            raise ValueError(f"voxel_downsample: {name} must be on the device (with xyz), it is on {t.device}")
    return M, voxel, int(min_count), slots


def voxel_downsample(xyz, voxel, priority=None, rgb=None, reduce="best", min_count=1, slots=0):
    """A point cloud reduced to one point per occupied cell of a grid of edge `voxel` (a3r_voxel_export, csrc/voxel.hip; include/a3r.h
    has the definition: float64 cells, the highest priority wins a cell and the lowest row an exact tie, integer sums for the mean --
    bitwise the numpy restatement).  xyz [M,3] float32, priority [M] float32 or None, rgb [M,3] uint8 or None: contiguous device
    tensors.  reduce: 'best' = the winner's own row, 'mean' = the unweighted mean of the cell's points and colours.  min_count: cells
    with fewer points are left out.  slots: 0 = a hash table of the smallest power of two >= 2 M entries, otherwise a power of two
    above M (the result does not depend on it).  Returns a dict: xyz [V,3] float32, rgb [V,3] uint8 (with rgb), index [V] int32 = the
    winner's row, ascending, count [V] int32 = the cell's points, and dropped = the number of points in no cell (non-finite, or
    beyond +-2^20 cells from the origin), a Python int.  One call into the library, which synchronises once to learn V; the outputs
    are written into M-row buffers and returned as V-row copies."""
    M, voxel, min_count, slots = _voxel_args(xyz, voxel, priority, rgb, reduce, min_count, slots)
    lib, dev, mode = _lib.load(), xyz.device, VOXEL_REDUCE[reduce]
    ws_bytes = int(lib.a3r_voxel_workspace_bytes(M, slots, mode))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    out_xyz = torch.empty((M, 3), dtype=torch.float32, device=dev)
    out_rgb = torch.empty((M, 3), dtype=torch.uint8, device=dev) if rgb is not None else None
    index = torch.empty(M, dtype=torch.int32, device=dev)
    count = torch.empty(M, dtype=torch.int32, device=dev)
    V, dropped = C.c_longlong(0), C.c_longlong(0)
    with torch.cuda.device(dev):
        check(lib.a3r_voxel_export(ptr(xyz), ptr(priority), ptr(rgb), M, voxel, mode, min_count, slots, ptr(ws), ws_bytes, M, ptr(out_xyz),
                                   ptr(out_rgb), ptr(index), ptr(count), C.byref(V), C.byref(dropped), stream_ptr()), "voxel_downsample")
    V = int(V.value)
    narrow = lambda t: t if V == M else t[:V].clone()
    out = dict(xyz=narrow(out_xyz))
    if out_rgb is not None:
        out["rgb"] = narrow(out_rgb)
    out.update(index=narrow(index), count=narrow(count), dropped=int(dropped.value))
    return out


def track_points(xyz, keep, flow_a, flow_b, steps, seeds=None, fb_thr=3.0):
    """Points followed through a clip by chaining optical-flow fields, read off the point maps at every frame they pass
    (a3r_track_points, csrc/track.hip; include/a3r.h has the definition: float64 bilinear samples, a track ends where it leaves the
    image or where forward and backward flow disagree by fb_thr pixels or more, the pixel by half-to-even rounding -- bitwise the
    numpy restatement).  xyz [N,H,W,3] float32, keep [N,H,W] uint8 or bool, flow_a / flow_b [E,2,H,W] float32: contiguous device
    tensors.  steps [C,S,4] (or [S,4]: one chain) integers, rows (frame_from, frame_to, edge, reversed): a host array, or a tensor
    anywhere (a device tensor is read back once for the entry checks).  seeds [M,2] float32 device tensor of (x, y), or None =
    every pixel.  Enqueue-only; returns a dict of device tensors xy [C,S+1,M,2] float32, xyz [C,S+1,M,3] float32, pix [C,S+1,M]
    int32 and state [C,S+1,M] uint8 (2 = visible, 1 = followed but not visible, 0 = ended)."""
    _req(xyz, "xyz"); _req(flow_a, "flow_a"); _req(flow_b, "flow_b")
    dev = xyz.device
    if xyz.dim() != 4 or xyz.shape[3] != 3:
        raise RuntimeError(f"track_points: xyz is [N,H,W,3], got {tuple(xyz.shape)}")
    N, H, W = xyz.shape[:3]
    if not (isinstance(keep, torch.Tensor) and keep.device == dev and keep.dtype in (torch.uint8, torch.bool) and keep.is_contiguous()
            and tuple(keep.shape) == (N, H, W)):
        raise RuntimeError("track_points: keep must be a contiguous uint8 or bool tensor [N,H,W] on xyz's device")
    if keep.dtype == torch.bool:
        keep = keep.view(torch.uint8)
    if not (flow_a.device == flow_b.device == dev and flow_a.dim() == 4 and tuple(flow_a.shape[1:]) == (2, H, W)
            and flow_b.shape == flow_a.shape):
        raise RuntimeError(f"track_points: flow_a / flow_b are [E,2,{H},{W}] on xyz's device, got {tuple(flow_a.shape)} and "
                           f"{tuple(flow_b.shape)}")
    E = flow_a.shape[0]
    st = steps.detach().cpu().numpy() if isinstance(steps, torch.Tensor) else np.asarray(steps)
    if st.ndim == 2:
        st = st[None]
    if st.ndim != 3 or st.shape[2] != 4 or st.dtype.kind not in "iu":
        raise ValueError(f"track_points: steps is an integer array [C,S,4] or [S,4], got {st.dtype} {st.shape}")
    if st.size and (st.min() < -(1 << 31) or st.max() >= (1 << 31)):
        raise ValueError("track_points: a step entry does not fit int32")
    st = np.ascontiguousarray(st, dtype=np.int32)
    Cn, S = st.shape[:2]
    if seeds is not None:
        _req(seeds, "seeds")
        if seeds.device != dev or seeds.dim() != 2 or seeds.shape[1] != 2:
            raise RuntimeError(f"track_points: seeds is [M,2] on xyz's device, got {tuple(seeds.shape)}")
    M = H * W if seeds is None else seeds.shape[0]
    lib = _lib.load()
    ok = Cn * (S + 1) * M < (1 << 31)                      # otherwise the call below refuses before it reads the outputs
    lead = (Cn, S + 1, M) if ok else (0, 0, 0)
    out = dict(xy=torch.empty(lead + (2,), dtype=torch.float32, device=dev), xyz=torch.empty(lead + (3,), dtype=torch.float32, device=dev),
               pix=torch.empty(lead, dtype=torch.int32, device=dev), state=torch.empty(lead, dtype=torch.uint8, device=dev))
    st_dev = torch.from_numpy(st.reshape(-1).copy()).to(dev) if st.size else None
    with torch.cuda.device(dev):
        check(lib.a3r_track_points(ptr(xyz), ptr(keep), N, H, W, ptr(flow_a), ptr(flow_b), E, ptr(st_dev), st.ctypes.data if st.size else None,
                                   Cn, S, ptr(seeds), M, float(fb_thr), ptr(out["xy"]), ptr(out["xyz"]), ptr(out["pix"]), ptr(out["state"]),
                                   stream_ptr()), "track_points")
    return out                                            # the device copy of the steps is freed stream-ordered after the kernel


def _tsdf_scalar(who, name, value):
    value = float(value)
    if not (np.isfinite(value) and value > 0):
        raise ValueError(f"{who}: {name} = {value} must be finite and positive")
    return value


def _tsdf_grid(who, origin, dims, voxel):
    """The grid's checks shared by tsdf_integrate and tsdf_mesh: (origin float64 [3], (nx, ny, nz), voxel)."""
    voxel = _tsdf_scalar(who, "voxel", voxel)
    origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(-1))
    if origin.shape != (3,) or not np.all(np.isfinite(origin)):
        raise ValueError(f"{who}: origin is three finite numbers, got {origin!r}")
    if len(dims) != 3 or any(int(n) != n or n <= 0 for n in dims):
        raise ValueError(f"{who}: dims = {tuple(dims)!r} is three positive integers (nx, ny, nz)")
    nx, ny, nz = (int(n) for n in dims)
    if nx * ny * nz >= 1 << 31:
        raise ValueError(f"{who}: dims = ({nx}, {ny}, {nz}): nx * ny * nz = {nx * ny * nz} must stay below 2^31")
    return origin, (nx, ny, nz), voxel


def _tsdf_tensor(who, t, name, dtype, shape):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{who}: {name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{who}: {name} must be {dtype}, got {t.dtype}")
    if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
        raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected {[w if w is not None else '*' for w in shape]}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous")


def _tsdf_devices(who, first, tensors):
    for t, name in tensors:
        if t is not None and (t.device.type != "cuda" or t.device != first.device):
            raise ValueError(f"{who}: {name} must be on the device (with {tensors[0][1]}), it is on {t.device}")


def tsdf_cameras(w2c, K, shapes):
    """The camera table of tsdf_integrate, [N,17] float64 (a3r_tsdf_cam: [R|t] row-major, fx, fy, cx, cy, then h and w as two int32 in
    the last column), from w2c [N,3,4] or [N,4,4] and K [N,3,3], both float64 (numpy or torch), and shapes = N pairs (h, w).  A
    non-zero skew, a non-finite entry and a non-positive shape are ValueErrors."""
    who = "tsdf_cameras"
    as_f64 = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    w2c, K = as_f64(w2c), as_f64(K)
    for a, name in ((w2c, "w2c"), (K, "K")):
        if a.dtype != np.float64:
            raise ValueError(f"{who}: {name} must be float64, got {a.dtype}")
    if w2c.ndim != 3 or w2c.shape[1] not in (3, 4) or w2c.shape[2] != 4:
        raise ValueError(f"{who}: w2c is [N,3,4] or [N,4,4], got {w2c.shape}")
    N = w2c.shape[0]
    if K.shape != (N, 3, 3):
        raise ValueError(f"{who}: K is [N,3,3] with N = {N}, got {K.shape}")
    if np.any(K[:, 0, 1] != 0):
        raise ValueError(f"{who}: K has a non-zero skew K[0,1]; the cameras are fx, fy, cx, cy")
    shapes = np.asarray(shapes)
    if shapes.shape != (N, 2) or np.any(shapes != shapes.astype(np.int64)) or np.any(shapes <= 0) or np.any(shapes >= 1 << 31):
        raise ValueError(f"{who}: shapes is N = {N} pairs (h, w) of positive integers, got {shapes.tolist()!r}")
    cams = np.zeros((N, 17), np.float64)
    cams[:, :12] = w2c[:, :3, :].reshape(N, 12)
    cams[:, 12], cams[:, 13], cams[:, 14], cams[:, 15] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    if not np.all(np.isfinite(cams[:, :16])):
        raise ValueError(f"{who}: w2c and K must be finite")
    cams[:, 16:].view(np.int32)[:] = shapes.astype(np.int32)
    return cams


def tsdf_camera_shapes(cams):
    """(h, w) per camera of a tsdf_cameras table, int32 [N,2]."""
    return np.ascontiguousarray(cams)[:, 16:].view(np.int32).copy()


def _tsdf_integrate_args(depth, weight, rgb, cams, origin, dims, voxel, trunc, near, max_depth):
    """The checks of tsdf_integrate; every refusal is a ValueError raised before the library is touched.  The scalars first, then
    every tensor's type, dtype, shape and layout, the camera table, the devices last."""
    who = "tsdf_integrate"
    origin, dims, voxel = _tsdf_grid(who, origin, dims, voxel)
    trunc = _tsdf_scalar(who, "trunc", trunc)
    near = _tsdf_scalar(who, "near", near)
    max_depth = float(max_depth)
    if not max_depth > 0:
        raise ValueError(f"{who}: max_depth = {max_depth} must be positive (inf = no limit)")
    _tsdf_tensor(who, depth, "depth", torch.float32, (None, None))
    N, P = depth.shape
    _tsdf_tensor(who, weight, "weight", torch.float32, (N, P))
    if rgb is not None:
        _tsdf_tensor(who, rgb, "rgb", torch.uint8, (N, P, 3))
    if N * P >= 1 << 31:
        raise ValueError(f"{who}: N * P = {N} * {P} must stay below 2^31")
    if not isinstance(cams, np.ndarray) or cams.dtype != np.float64 or cams.shape != (N, 17):
        raise ValueError(f"{who}: cams is the float64 table [N,17] of tsdf_cameras with N = {N}, got "
                         f"{getattr(cams, 'shape', type(cams).__name__)}")
    cams = np.ascontiguousarray(cams)
    if not np.all(np.isfinite(cams[:, :16])):
        raise ValueError(f"{who}: cams holds a non-finite entry")
    for n, (h, w) in enumerate(tsdf_camera_shapes(cams).tolist()):
        if h <= 0 or w <= 0 or h * w > P:
            raise ValueError(f"{who}: camera {n}: h * w = {h} * {w} must be positive and at most P = {P}")
    _tsdf_devices(who, depth, [(depth, "depth"), (weight, "weight"), (rgb, "rgb")])
    return cams, origin, dims, voxel, trunc, near, max_depth


def tsdf_integrate(depth, weight, rgb, cams, origin, dims, voxel, trunc, near=1e-6, max_depth=float("inf"), skip_stats=None):
    """Depth maps fused into a dense grid of truncated signed distances (a3r_tsdf_integrate, csrc/tsdf.hip; include/a3r.h has the
    definition: float64, every voxel walks the frames in ascending order with its sums in registers -- bitwise the numpy
    restatement).  depth, weight [N,P] float32 and rgb [N,P,3] uint8 or None: contiguous device tensors, pixel (row, col) of frame n
    at n * P + row * w + col; cams: the table of tsdf_cameras(); origin (3 numbers), dims = (nx, ny, nz), voxel, trunc, near,
    max_depth: the grid and the gates.  skip_stats: None or a device tensor of two int64 the call adds its brick-test counts to.
    Enqueue-only; returns device tensors tsdf [nz,ny,nx] float32 (1 where nothing was seen), wsum [nz,ny,nx] float32 and
    rgb [nz,ny,nx,3] uint8 (None without rgb)."""
    cams, origin, (nx, ny, nz), voxel, trunc, near, max_depth = _tsdf_integrate_args(depth, weight, rgb, cams, origin, dims, voxel, trunc,
                                                                                     near, max_depth)
    if skip_stats is not None:
        _tsdf_tensor("tsdf_integrate", skip_stats, "skip_stats", torch.int64, (2,))
        _tsdf_devices("tsdf_integrate", depth, [(depth, "depth"), (skip_stats, "skip_stats")])
    assert C.sizeof(_lib.TsdfCam) == 136 == cams.shape[1] * cams.itemsize
    lib, dev, (N, P) = _lib.load(), depth.device, depth.shape
    tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
    wsum = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
    out_rgb = torch.empty((nz, ny, nx, 3), dtype=torch.uint8, device=dev) if rgb is not None else None
    cams_dev = torch.from_numpy(cams.reshape(-1).copy()).to(dev) if N else None
    with torch.cuda.device(dev):
        check(lib.a3r_tsdf_integrate(ptr(depth), ptr(weight), ptr(rgb), ptr(cams_dev), cams.ctypes.data if N else None, N, P,
                                     origin.ctypes.data, voxel, nx, ny, nz, trunc, near, max_depth, ptr(tsdf), ptr(wsum), ptr(out_rgb),
                                     ptr(skip_stats), stream_ptr()), "tsdf_integrate")
    return tsdf, wsum, out_rgb            # the camera table is freed stream-ordered after the kernel


def tsdf_set_form(form):
    """a3r_tsdf_set_form: bit 0 set = no brick test; returns the previous form.  The outputs do not depend on it."""
    return int(_lib.load().a3r_tsdf_set_form(int(form)))


def _tsdf_mesh_args(tsdf, wsum, rgb, origin, voxel, min_weight):
    who = "tsdf_mesh"
    min_weight = _tsdf_scalar(who, "min_weight", min_weight)
    _tsdf_tensor(who, tsdf, "tsdf", torch.float32, (None, None, None))
    nz, ny, nx = tsdf.shape
    origin, dims, voxel = _tsdf_grid(who, origin, (nx, ny, nz), voxel)
    if nx * ny * nz > (1 << 31) // 6:
        raise ValueError(f"{who}: dims = ({nx}, {ny}, {nz}): more than 2^31 / 6 voxels (the face count is a 32-bit integer)")
    _tsdf_tensor(who, wsum, "wsum", torch.float32, (nz, ny, nx))
    if rgb is not None:
        _tsdf_tensor(who, rgb, "rgb", torch.uint8, (nz, ny, nx, 3))
    _tsdf_devices(who, tsdf, [(tsdf, "tsdf"), (wsum, "wsum"), (rgb, "rgb")])
    return origin, dims, voxel, min_weight


def tsdf_mesh(tsdf, wsum, rgb, origin, voxel, min_weight, capacity=None):
    """The zero surface of a TSDF grid as one triangle mesh by surface nets (a3r_tsdf_mesh_count / _export, csrc/tsdf.hip;
    include/a3r.h has the definition -- bitwise the numpy restatement).  tsdf, wsum [nz,ny,nx] float32 and rgb [nz,ny,nx,3] uint8 or
    None as tsdf_integrate returned them; a voxel counts as observed where wsum >= min_weight.  Returns device tensors xyz [V,3]
    float32, rgb [V,3] uint8 (None without rgb) and faces [F,3] int32.  Two calls into the library, each synchronising once;
    capacity = (vertices, faces) skips the first and is refused by the second when it is too small."""
    origin, (nx, ny, nz), voxel, min_weight = _tsdf_mesh_args(tsdf, wsum, rgb, origin, voxel, min_weight)
    lib, dev = _lib.load(), tsdf.device
    ws_bytes = int(lib.a3r_tsdf_mesh_workspace_bytes(nx, ny, nz))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    V, F = C.c_longlong(0), C.c_longlong(0)
    with torch.cuda.device(dev):
        if capacity is None:
            check(lib.a3r_tsdf_mesh_count(ptr(tsdf), ptr(wsum), nx, ny, nz, min_weight, ptr(ws), ws_bytes, C.byref(V), C.byref(F),
                                          stream_ptr()), "tsdf_mesh")
            capacity = (int(V.value), int(F.value))
        cap_v, cap_f = int(capacity[0]), int(capacity[1])
        xyz = torch.empty((cap_v, 3), dtype=torch.float32, device=dev)
        out_rgb = torch.empty((cap_v, 3), dtype=torch.uint8, device=dev) if rgb is not None else None
        faces = torch.empty((cap_f, 3), dtype=torch.int32, device=dev)
        check(lib.a3r_tsdf_mesh_export(ptr(tsdf), ptr(wsum), ptr(rgb), nx, ny, nz, origin.ctypes.data, voxel, min_weight, ptr(ws), ws_bytes,
                                       cap_v, cap_f, ptr(xyz) if cap_v else None, ptr(out_rgb) if cap_v else None,
                                       ptr(faces) if cap_f else None, C.byref(V), C.byref(F), stream_ptr()), "tsdf_mesh")
    V, F = int(V.value), int(F.value)
    return xyz[:V], (out_rgb[:V] if out_rgb is not None else None), faces[:F]
