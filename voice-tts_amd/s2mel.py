"""PyTorch glue for the semantic-to-mel stage -- `north_star`: "PyTorch-ROCm hosts the
tensors and the s2mel/vqvae glue".  Functional restatement (weights in a flat dict keyed like the reference's
state dicts, weight norm folded at load) of

  infer_v2.py:713-731                      gpt_layer -> vq2emb + latent -> length_regulator -> cat(prompt) -> CFM -> crop
  s2mel/modules/commons.py:388-438         MyModel (`models.{gpt_layer,length_regulator,cfm}`)
  s2mel/modules/length_regulator.py:28-141 InterpolateRegulator (continuous input, nearest interpolation)
  s2mel/modules/flow_matching.py:30-115    BASECFM.inference / solve_euler (CFG batch-2 stacking)
  s2mel/modules/diffusion_transformer.py:103-257  DiT (U-ViT skips, long skip, WaveNet head)
  s2mel/modules/gpt_fast/model.py:121-360  Transformer / AdaptiveLayerNorm(RMSNorm) / RoPE attention / SwiGLU
  s2mel/modules/wavenet.py:103-174 + encodec.py:192-228  WN with reflect-padded weight-normed convs
  utils/maskgct/.../factorized_vector_quantize.py:99-127  vq2emb = out_project(codebook[ids])

Runs on whatever device its tensors live on (GPU in the pipeline; CPU in the parity tests).  The CFM noise is an
explicit argument so CPU/GPU runs can share it.
"""
import math
import os

import torch
import torch.nn.functional as F

from . import gemm as G
from .convs import conv1d  # GEMM forms: no MIOpen in the request path (convs.py)

from .weights import fold_weight_norm

S2MEL_CFG = dict(
    hidden_dim=512, num_heads=8, depth=13, in_channels=80, content_dim=512, style_dim=192,
    wavenet_hidden=512, wavenet_layers=8, wavenet_kernel=5, wavenet_dilation_rate=1,
    lr_channels=512, lr_in_channels=1024, lr_n_blocks=4, gpt_dim=1280, codebook_dim=8, codebook_size=8192, semantic_dim=1024,
)


FRAMES_PER_CODE = 1.72  # mel frames (22 050 Hz, hop 256) per semantic code at the natural pace (infer_v2.py:719)
SPEED_RANGE = (0.5, 2.0)  # an interface condition, not a measurement: at 0.5 the nearest-neighbour regulator repeats every code frame 3-4 times


def check_speed(speed):
    """-> None, or `speed` as a float; ValueError for a bool, a NaN, anything that is not a number and a value outside `SPEED_RANGE`."""
    if speed is None:
        return None
    lo, hi = SPEED_RANGE
    if isinstance(speed, bool) or not isinstance(speed, (int, float)) or not lo <= float(speed) <= hi:  # (NaN fails the comparison)
        raise ValueError(f"speed {speed!r} is not a number in [{lo:g}, {hi:g}]")
    return float(speed)


def target_frames(n_codes, speed=None):
    """Mel frames the length regulator stretches `n_codes` codes to: THE definition (`S2Mel`, the pinned noise, `audio_seconds`).
    `speed` None: `(code_lens * 1.72).long()` as the reference evaluates it (infer_v2.py:719) -- an integer tensor times a Python
    float in torch's default dtype.  Otherwise `(code_lens * 1.72 / speed).long()`, at least 1 frame (1 code at speed 2.0 truncates
    to 0).  More frames per code is a slower tempo at the same pitch: the vocoder still sees 22 050 Hz mels.  A tensor of lengths
    gives a tensor (same device), an int an int."""
    code_lens = n_codes if torch.is_tensor(n_codes) else torch.tensor([int(n_codes)])
    if speed is None:
        frames = (code_lens * FRAMES_PER_CODE).long()
    else:
        frames = (code_lens * FRAMES_PER_CODE / speed).long().clamp_(min=1)
    return frames if torch.is_tensor(n_codes) else int(frames)


def tiny_s2mel_cfg(**kw):
    c = dict(S2MEL_CFG)
    c.update(hidden_dim=64, num_heads=2, depth=5, content_dim=32, style_dim=12, wavenet_hidden=64, wavenet_layers=3,
             lr_channels=32, lr_in_channels=40, lr_n_blocks=2, gpt_dim=128, codebook_size=8194, semantic_dim=40)
    c.update(kw)
    return c


def _ffn_dim(dim):
    n_hidden = int(2 * (4 * dim) / 3)
    return n_hidden if n_hidden % 256 == 0 else n_hidden + 256 - (n_hidden % 256)


def s2mel_shapes(cfg=S2MEL_CFG):
    """(name, shape) of every tensor (weight norm already folded)."""
    H, Hw, C = cfg["hidden_dim"], cfg["wavenet_hidden"], cfg["in_channels"]
    assert H == Hw, "FinalLayer's adaLN takes the DiT timestep embedding: wavenet.hidden_dim must equal DiT.hidden_dim"
    out = [("gpt_layer.0.weight", (256, cfg["gpt_dim"])), ("gpt_layer.0.bias", (256,)), ("gpt_layer.1.weight", (128, 256)),
           ("gpt_layer.1.bias", (128,)), ("gpt_layer.2.weight", (cfg["semantic_dim"], 128)), ("gpt_layer.2.bias", (cfg["semantic_dim"],)),
           ("quantizer.codebook.weight", (cfg["codebook_size"], cfg["codebook_dim"])),
           ("quantizer.out_project.weight", (cfg["semantic_dim"], cfg["codebook_dim"], 1)), ("quantizer.out_project.bias", (cfg["semantic_dim"],))]
    lr = cfg["lr_channels"]
    out += [("length_regulator.content_in_proj.weight", (lr, cfg["lr_in_channels"])), ("length_regulator.content_in_proj.bias", (lr,))]
    for i in range(cfg["lr_n_blocks"]):
        out += [(f"length_regulator.model.{3 * i}.weight", (lr, lr, 3)), (f"length_regulator.model.{3 * i}.bias", (lr,)),
                (f"length_regulator.model.{3 * i + 1}.weight", (lr,)), (f"length_regulator.model.{3 * i + 1}.bias", (lr,))]
    n = 3 * cfg["lr_n_blocks"]
    out += [(f"length_regulator.model.{n}.weight", (lr, lr, 1)), (f"length_regulator.model.{n}.bias", (lr,))]
    e = "cfm.estimator."
    out += [(e + "t_embedder.mlp.0.weight", (H, 256)), (e + "t_embedder.mlp.0.bias", (H,)), (e + "t_embedder.mlp.2.weight", (H, H)), (e + "t_embedder.mlp.2.bias", (H,)),
            (e + "t_embedder2.mlp.0.weight", (Hw, 256)), (e + "t_embedder2.mlp.0.bias", (Hw,)), (e + "t_embedder2.mlp.2.weight", (Hw, Hw)), (e + "t_embedder2.mlp.2.bias", (Hw,)),
            (e + "cond_projection.weight", (H, cfg["content_dim"])), (e + "cond_projection.bias", (H,)),
            (e + "cond_x_merge_linear.weight", (H, H + 2 * C + cfg["style_dim"])), (e + "cond_x_merge_linear.bias", (H,)),
            (e + "skip_linear.weight", (H, H + C)), (e + "skip_linear.bias", (H,)),
            (e + "conv1.weight", (Hw, H)), (e + "conv1.bias", (Hw,)), (e + "conv2.weight", (C, Hw, 1)), (e + "conv2.bias", (C,)),
            (e + "res_projection.weight", (Hw, H)), (e + "res_projection.bias", (Hw,)),
            (e + "final_layer.linear.weight", (Hw, Hw)), (e + "final_layer.linear.bias", (Hw,)),
            (e + "final_layer.adaLN_modulation.1.weight", (2 * Hw, Hw)), (e + "final_layer.adaLN_modulation.1.bias", (2 * Hw,))]
    t = e + "transformer."
    inter = _ffn_dim(H)
    for i in range(cfg["depth"]):
        p = t + f"layers.{i}."
        out += [(p + "attention.wqkv.weight", (3 * H, H)), (p + "attention.wo.weight", (H, H)),
                (p + "feed_forward.w1.weight", (inter, H)), (p + "feed_forward.w3.weight", (inter, H)), (p + "feed_forward.w2.weight", (H, inter)),
                (p + "ffn_norm.project_layer.weight", (2 * H, H)), (p + "ffn_norm.project_layer.bias", (2 * H,)), (p + "ffn_norm.norm.weight", (H,)),
                (p + "attention_norm.project_layer.weight", (2 * H, H)), (p + "attention_norm.project_layer.bias", (2 * H,)), (p + "attention_norm.norm.weight", (H,)),
                (p + "skip_in_linear.weight", (H, 2 * H)), (p + "skip_in_linear.bias", (H,))]
    out += [(t + "norm.project_layer.weight", (2 * H, H)), (t + "norm.project_layer.bias", (2 * H,)), (t + "norm.norm.weight", (H,))]
    w = e + "wavenet."
    nl, k = cfg["wavenet_layers"], cfg["wavenet_kernel"]
    out += [(w + "cond_layer.conv.conv.weight", (2 * Hw * nl, Hw, 1)), (w + "cond_layer.conv.conv.bias", (2 * Hw * nl,))]
    for i in range(nl):
        rs = 2 * Hw if i < nl - 1 else Hw
        out += [(w + f"in_layers.{i}.conv.conv.weight", (2 * Hw, Hw, k)), (w + f"in_layers.{i}.conv.conv.bias", (2 * Hw,)),
                (w + f"res_skip_layers.{i}.conv.conv.weight", (rs, Hw, 1)), (w + f"res_skip_layers.{i}.conv.conv.bias", (rs,))]
    return out


def make_s2mel_weights(cfg=S2MEL_CFG, seed=1234):
    """Seeded synthetic weights (no checkpoint exists offline): N(0, 1/fan_in) matrices, small biases, gains near 1."""
    g = torch.Generator().manual_seed(seed)
    W = {}
    for name, shape in s2mel_shapes(cfg):
        if name.endswith("norm.weight") or (".model." in name and len(shape) == 1 and name.endswith(".weight")):
            W[name] = 1.0 + 0.1 * torch.randn(*shape, generator=g)
        elif name.endswith(".bias"):
            W[name] = 0.02 * torch.randn(*shape, generator=g)
        elif name == "quantizer.codebook.weight":
            W[name] = torch.randn(*shape, generator=g)
        else:
            fan = 1
            for d in shape[1:]:
                fan *= d
            W[name] = torch.randn(*shape, generator=g) / math.sqrt(fan)
    return W


def _pad_reflect(x, left, right):
    """encodec.pad1d(mode='reflect'): zero-extend first when the input is shorter than the pad (encodec.py:96-113)."""
    L = x.shape[-1]
    extra = 0
    if L <= max(left, right):
        extra = max(left, right) - L + 1
        x = F.pad(x, (0, extra))
    y = F.pad(x, (left, right), mode="reflect")
    return y[..., : y.shape[-1] - extra]


def attn_full(q, k, v, scale=None, rope=None):
    """softmax(scale * q k^T) v for q, k, v [B, T, h, 64] fp32 CUDA tensors (any strides with d contiguous) through
    libixtts_hip.so's fp32-MFMA flash kernel (csrc/attn_full.hip); returns [B, T, h, 64] contiguous.
    rope: complex64 [>= T, 32] -- q and k come unrotated and the kernel rotates them as it splits them (csrc/attn_full_x3.hip; not
    with IXTTS_ATTN_FULL=f32): the bits of `ixtts_rope_qk_f32` followed by this call without `rope`."""
    import ctypes as C

    from . import _lib

    B, T, Hh, d = q.shape
    assert d == 64 and q.is_cuda and q.dtype == torch.float32 and k.shape == q.shape and v.shape == q.shape
    for t in (q, k, v):
        assert t.stride(3) == 1 and t.stride() == q.stride() and t.stride(1) % 4 == 0 and t.data_ptr() % 16 == 0
    out = torch.empty(B, T, Hh, d, device=q.device, dtype=torch.float32)
    sc = float(scale if scale is not None else 1.0 / math.sqrt(d))
    L = _lib.lib()
    nws = L.ixtts_attn_full_workspace_bytes(B, Hh, T)
    ws = torch.empty(nws, device=q.device, dtype=torch.uint8)  # scratch for the key-split partials (caching allocator: no hipMalloc)
    with torch.cuda.device(q.device):
        if rope is not None:
            assert rope.dtype == torch.complex64 and rope.is_contiguous() and rope.shape[0] >= T and rope.shape[1] == d // 2
            rc = L.ixtts_attn_full_rope_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), torch.view_as_real(rope).data_ptr(), rope.shape[0], B, Hh,
                                            T, d, q.stride(0), q.stride(1), q.stride(2), out.stride(0), out.stride(1), out.stride(2), C.c_float(sc),
                                            ws.data_ptr(), nws, _lib.current_stream_ptr())
        else:
            rc = L.ixtts_attn_full_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, Hh, T, d, q.stride(0), q.stride(1),
                                       q.stride(2), out.stride(0), out.stride(1), out.stride(2), C.c_float(sc), ws.data_ptr(), nws,
                                       _lib.current_stream_ptr())
    _lib.check(rc, "ixtts_attn_full_rope_f32" if rope is not None else "ixtts_attn_full_f32")
    return out


def _lin(x, W, name):
    return F.linear(x, W[name + ".weight"], W.get(name + ".bias"))


# ---------------------------------------------------------------------------------- fused row / element ops
# On the GPU these are single HIP passes (csrc/dit_ops.hip, declared in include/ixtts_hip.h); on the CPU (parity tests
# against the reference's modules) the same arithmetic in torch.
def _hip_call(name, *args):
    from . import _lib

    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()), name)


def adaln_rmsnorm(x, wb, g, eps=1e-5):
    """AdaptiveLayerNorm over RMSNorm (gpt_fast/model.py:18-37,362-372): x [B,T,H], wb = project_layer(c) [B,2H] (weight | bias)."""
    B, T, H = x.shape
    if x.is_cuda:
        import ctypes as C

        x, wb = x.contiguous(), wb.contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _hip_call("ixtts_adaln_rmsnorm_f32", x.data_ptr(), wb.data_ptr(), g.data_ptr(), out.data_ptr(), B, T, H, C.c_float(eps))
        return out
    w, b = wb[:, None, :H], wb[:, None, H:]
    return torch.addcmul(b, w, F.rms_norm(x, (H,), g, eps))


def adaln_rmsnorm_planes(x, wb, g, eps=1e-5, pk=None):
    """`adaln_rmsnorm` (pk: `adaln_rmsnorm_packed`) for a consumer that is a split-product GEMM: the norm's rows as `G.Planes`, written
    by the norm kernel itself -- the bytes `G.split` makes of the fp32 rows, which are not written.  Device only; H % 64 == 0."""
    import ctypes as C

    H = x.shape[-1]
    rows = x.numel() // H
    x, wb = x.contiguous(), wb.contiguous()
    buf = G.planes_buffer(rows, H, x.device)
    with torch.cuda.device(x.device):
        if pk is None:
            B, T, _ = x.shape
            _hip_call("ixtts_adaln_rmsnorm_planes_f32", x.data_ptr(), wb.data_ptr(), g.data_ptr(), buf.data_ptr(), B, T, H, C.c_float(eps))
        else:
            _hip_call("ixtts_adaln_rmsnorm_planes_varlen_f32", x.data_ptr(), wb.data_ptr(), g.data_ptr(), buf.data_ptr(), pk.tab.data_ptr(), pk.n, rows, H,
                      C.c_float(eps))
    return G.Planes(buf, rows, H)


def ln_modulate(x, ss, eps=1e-6):
    """FinalLayer: layer_norm(x, no affine) * (1 + scale) + shift, ss = adaLN_modulation(c) [B,2H] = (shift | scale)."""
    B, T, H = x.shape
    if x.is_cuda:
        import ctypes as C

        x, ss = x.contiguous(), ss.contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _hip_call("ixtts_ln_modulate_f32", x.data_ptr(), ss.data_ptr(), out.data_ptr(), B, T, H, C.c_float(eps))
        return out
    return F.layer_norm(x, (H,), None, None, eps) * (1 + ss[:, None, H:]) + ss[:, None, :H]


def swiglu(u):
    """silu(u[..., :F]) * u[..., F:] on the fused [w1; w3] GEMM output (gpt_fast/model.py:316-326)."""
    Fd = u.shape[-1] // 2
    if u.is_cuda:
        u = u.contiguous()
        out = torch.empty(*u.shape[:-1], Fd, device=u.device, dtype=u.dtype)
        with torch.cuda.device(u.device):
            _hip_call("ixtts_swiglu_f32", u.data_ptr(), out.data_ptr(), u.numel() // (2 * Fd), Fd)
        return out
    return F.silu(u[..., :Fd]) * u[..., Fd:]


def wn_gate(a, g, off, C_):
    """tanh(a[:, :C] + g_a) * sigmoid(a[:, C:] + g_b) with (g_a | g_b) = g[:, off:off+2C] (wavenet.py:142-160)."""
    B, _, T = a.shape
    if a.is_cuda:
        a, g = a.contiguous(), g.contiguous()
        out = torch.empty(B, C_, T, device=a.device, dtype=a.dtype)
        with torch.cuda.device(a.device):
            _hip_call("ixtts_wn_gate_f32", a.data_ptr(), g.data_ptr(), out.data_ptr(), B, C_, T, g.shape[1], off)
        return out
    x = a + g[:, off:off + 2 * C_, None]
    return torch.tanh(x[:, :C_]) * torch.sigmoid(x[:, C_:])


def wn_gate_rows(a, g, off, C_, rows_per_batch):
    """`wn_gate` in row layout: a [rows, 2C] -> [rows, C]; row r uses the gate biases of batch entry min(r // rows_per_batch, B-1)."""
    rows, B = a.shape[0], g.shape[0]
    if a.is_cuda:
        a, g = a.contiguous(), g.contiguous()
        out = torch.empty(rows, C_, device=a.device, dtype=a.dtype)
        with torch.cuda.device(a.device):
            _hip_call("ixtts_wn_gate_rows_f32", a.data_ptr(), g.data_ptr(), out.data_ptr(), rows, C_, rows_per_batch, B, g.shape[1], off)
        return out
    b = (torch.arange(rows, device=a.device) // rows_per_batch).clamp(max=B - 1)
    x = a + g[b, off:off + 2 * C_]
    return torch.tanh(x[:, :C_]) * torch.sigmoid(x[:, C_:])


def reflect_halo_rows(p, T, left, right):
    """Refresh, in place, the reflect padding of p [B, left+T+right, C] from its interior rows."""
    B, _, C_ = p.shape
    if p.is_cuda:
        assert p.is_contiguous()
        with torch.cuda.device(p.device):
            _hip_call("ixtts_reflect_halo_rows_f32", p.data_ptr(), B, T, C_, left, right)
        return p
    if left:
        p[:, :left] = p[:, left + 1:2 * left + 1].flip(1)
    if right:
        p[:, left + T:] = p[:, left + T - 1 - right:left + T - 1].flip(1)
    return p


# ---------------------------------------------------------------------------------- packed (ragged) sequences
# n sequences of unequal length back to back as rows; sequence s owns rows [off[s], off[s+1]).  The GPU forms are the *_varlen HIP
# entries (csrc/dit_ops.hip, attn_full_x3.hip, gemm_x6.hip) reading a small int32 offsets table uploaded once per solve; the CPU forms
# are the same arithmetic through row -> sequence index gathers.
class RowPack:
    """Host description of a pack: `lens` (>= 1 each), `off` (n + 1 prefix sums).  `tab` int32 on `device` = [off | tile_off | (seq,
    128-query block) pairs] (the attention's table; its first n + 1 entries are the offsets every row op reads); CPU: `seq` / `pos`,
    each row's sequence and its position in it."""

    def __init__(self, lens, device):
        self.lens = [int(t) for t in lens]
        assert self.lens and min(self.lens) >= 1, self.lens
        self.n = len(self.lens)
        self.off = [0]
        for t in self.lens:
            self.off.append(self.off[-1] + t)
        self.rows = self.off[-1]
        self.device = torch.device(device)
        tiles = [0]
        for t in self.lens:
            tiles.append(tiles[-1] + (t + 63) // 64)
        self.tiles = tiles[-1]
        work = [(s, q) for s, t in enumerate(self.lens) for q in range((t + 127) // 128)]
        self.n_work = len(work)
        host = torch.tensor(self.off + tiles + [v for w in work for v in w], dtype=torch.int32)
        self.tab = host.to(self.device)
        if self.device.type != "cuda":
            self.seq = torch.repeat_interleave(torch.arange(self.n), torch.tensor(self.lens))
            self.pos = torch.arange(self.rows) - torch.tensor(self.off[:-1])[self.seq]

    def span(self, s):
        return self.off[s], self.off[s + 1]


def adaln_rmsnorm_packed(x, wb, g, pk, eps=1e-5):
    """`adaln_rmsnorm` over a pack: x [rows, H], wb [n, 2H]; row r takes the (weight | bias) row of its own sequence."""
    rows, H = x.shape
    if x.is_cuda:
        import ctypes as C

        x, wb = x.contiguous(), wb.contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _hip_call("ixtts_adaln_rmsnorm_varlen_f32", x.data_ptr(), wb.data_ptr(), g.data_ptr(), out.data_ptr(), pk.tab.data_ptr(), pk.n, rows, H, C.c_float(eps))
        return out
    wbr = wb[pk.seq]
    return torch.addcmul(wbr[:, H:], wbr[:, :H], F.rms_norm(x, (H,), g, eps))


def ln_modulate_packed(x, ss, pk, eps=1e-6):
    """`ln_modulate` over a pack: x [rows, H], ss [n, 2H] (shift | scale) per sequence."""
    rows, H = x.shape
    if x.is_cuda:
        import ctypes as C

        x, ss = x.contiguous(), ss.contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _hip_call("ixtts_ln_modulate_varlen_f32", x.data_ptr(), ss.data_ptr(), out.data_ptr(), pk.tab.data_ptr(), pk.n, rows, H, C.c_float(eps))
        return out
    ssr = ss[pk.seq]
    return F.layer_norm(x, (H,), None, None, eps) * (1 + ssr[:, H:]) + ssr[:, :H]


def rope_qk_packed(qkv, fc, pk, head_dim):
    """RoPE on the q and k thirds of a packed wqkv output qkv [rows, 3H], positions restarting at 0 in each sequence; fc complex
    [>= max len, head_dim / 2].  Device: in place (returns qkv).  CPU: returns a rotated copy."""
    rows, H3 = qkv.shape
    H = H3 // 3
    if qkv.is_cuda:
        assert qkv.is_contiguous() and fc.shape[0] >= max(pk.lens)
        with torch.cuda.device(qkv.device):
            _hip_call("ixtts_rope_qk_varlen_f32", qkv.data_ptr(), torch.view_as_real(fc).data_ptr(), pk.tab.data_ptr(), pk.n, rows, H, head_dim)
        return qkv
    f = fc[pk.pos][:, None, :]  # [rows, 1, hd/2]
    out = qkv.clone()
    for j in range(2):
        xc = torch.view_as_complex(qkv[:, j * H:(j + 1) * H].reshape(rows, H // head_dim, head_dim // 2, 2).contiguous())
        out[:, j * H:(j + 1) * H] = torch.view_as_real(xc * f).reshape(rows, H)
    return out


def attn_full_packed(q, k, v, pk, scale=None, rope=None):
    """softmax(scale q k^T) v per sequence of a pack: q, k, v [rows, h, 64] strided views (d contiguous, one row stride) of device fp32
    rows; queries of sequence s see the keys of sequence s only (csrc/attn_full_x3.hip, varlen entry).  Returns [rows, h, 64].
    rope: as `attn_full` (positions restart at 0 in each sequence; the table covers the longest)."""
    import ctypes as C

    from . import _lib

    rows, Hh, d = q.shape
    assert d == 64 and q.is_cuda and q.dtype == torch.float32 and k.shape == q.shape and v.shape == q.shape and rows == pk.rows
    for t in (q, k, v):
        assert t.stride(2) == 1 and t.stride() == q.stride() and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
    out = torch.empty(rows, Hh, d, device=q.device, dtype=torch.float32)
    sc = float(scale if scale is not None else 1.0 / math.sqrt(d))
    L = _lib.lib()
    nws = L.ixtts_attn_full_varlen_workspace_bytes(pk.n, Hh, pk.tiles)
    ws = torch.empty(nws, device=q.device, dtype=torch.uint8)
    with torch.cuda.device(q.device):
        if rope is not None:
            assert rope.dtype == torch.complex64 and rope.is_contiguous() and rope.shape[0] >= max(pk.lens) and rope.shape[1] == d // 2
            rc = L.ixtts_attn_full_rope_varlen_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), torch.view_as_real(rope).data_ptr(),
                                                   pk.tab.data_ptr(), pk.n, pk.tiles, pk.n_work, Hh, d, q.stride(0), q.stride(1), out.stride(0), out.stride(1),
                                                   C.c_float(sc), ws.data_ptr(), nws, _lib.current_stream_ptr())
        else:
            rc = L.ixtts_attn_full_varlen_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), pk.tab.data_ptr(), pk.n, pk.tiles, pk.n_work, Hh, d,
                                              q.stride(0), q.stride(1), out.stride(0), out.stride(1), C.c_float(sc), ws.data_ptr(), nws,
                                              _lib.current_stream_ptr())
    _lib.check(rc, "ixtts_attn_full_rope_varlen_f32" if rope is not None else "ixtts_attn_full_varlen_f32")
    return out


def wn_gate_rows_packed(a, g, off, C_, poff):
    """`wn_gate_rows` over the WaveNet's padded pack: row r takes the gate biases of the sequence s with poff[s] <= r < poff[s+1]
    (rows past the end: the last sequence).  poff: a RowPack of the padded lengths."""
    rows = a.shape[0]
    if a.is_cuda:
        a, g = a.contiguous(), g.contiguous()
        out = torch.empty(rows, C_, device=a.device, dtype=a.dtype)
        with torch.cuda.device(a.device):
            _hip_call("ixtts_wn_gate_rows_varlen_f32", a.data_ptr(), g.data_ptr(), out.data_ptr(), rows, C_, poff.tab.data_ptr(), poff.n, g.shape[1], off)
        return out
    b = torch.cat([poff.seq, poff.seq.new_full((max(0, rows - poff.rows),), poff.n - 1)])[:rows]
    x = a + g[b, off:off + 2 * C_]
    return torch.tanh(x[:, :C_]) * torch.sigmoid(x[:, C_:])


def _reflect_src(T, left, right):
    """Row sources of one sequence's halo under `_pad_reflect` (zero-extension included): (dst rows, src rows or -1 for zero)."""
    idx = _pad_reflect(torch.arange(1, T + 1, dtype=torch.float64)[None, None], left, right)[0, 0].long() - 1
    dst = list(range(left)) + list(range(left + T, left + T + right))
    return dst, [int(idx[i]) + left if int(idx[i]) >= 0 else -1 for i in dst]


def reflect_halo_rows_packed(p, poff, left, right):
    """Refresh, in place, the reflect halo of every sequence of the padded pack p [rows, C] (sequence s = left halo | interior |
    right halo over rows [poff[s], poff[s+1]))."""
    if p.is_cuda:
        assert p.is_contiguous() and min(poff.lens) - left - right > max(left, right)
        with torch.cuda.device(p.device):
            _hip_call("ixtts_reflect_halo_rows_varlen_f32", p.data_ptr(), poff.tab.data_ptr(), poff.n, p.shape[1], left, right)
        return p
    if not hasattr(poff, "halo"):
        dst, src, zero = [], [], []
        for s, L in enumerate(poff.lens):
            o = poff.off[s]
            for d_, s_ in zip(*_reflect_src(L - left - right, left, right)):
                (dst.append(o + d_), src.append(o + s_)) if s_ >= 0 else zero.append(o + d_)
        poff.halo = (torch.tensor(dst, dtype=torch.long), torch.tensor(src, dtype=torch.long), torch.tensor(zero, dtype=torch.long))
    dst, src, zero = poff.halo
    p[dst] = p[src]
    if zero.numel():
        p[zero] = 0
    return p


# Frames (sum of segment lengths, prompt frames included) per packed CFM solve (`S2Mel.solve_many`; IXTTS_S2MEL_BATCH_FRAMES): peak
# activations are ~0.1 MB per frame at production width, so a pack of this size holds ~1.6 GB
S2MEL_BATCH_FRAMES = 16384

TUNED_GEMMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunable", "gfx950_s2mel.csv")


def use_tuned_gemms(path=TUNED_GEMMS):
    """Library-GEMM selection for the DiT's fp32 GEMMs: PyTorch's TunableOp picks, per (layout, M, N, K), the fastest
    hipBLASLt / rocBLAS solution from a results file recorded on an MI355X with `tools/tune_gemms.py` (production shapes,
    T = 430 + 1892: wqkv 79 -> 56 us, [w1; w3] 136 -> 106 us, wo 40 -> 26 us).  Shapes without an entry keep the default
    heuristic; `IXTTS_TUNE=1` tunes new shapes online (seconds per shape, once).  Returns True when the file was taken."""
    if not torch.cuda.is_available():
        return False
    import torch.cuda.tunable as tn

    tn.enable(True)
    tn.tuning_enable(os.environ.get("IXTTS_TUNE") == "1")
    try:
        import tempfile

        tn.set_filename(os.path.join(tempfile.gettempdir(), "ixtts_tunableop_online.csv"))  # where online tuning (if on) records
    except Exception:
        pass
    try:
        return bool(os.path.isfile(path) and tn.read_file(path))
    except Exception:  # a file recorded under other library versions is refused by its validators: default heuristics
        return False


# The shipped results were recorded at ONE segment length (T = 430 prompt + 1892 target frames; the WaveNet head on Th = 1909 of them):
# TunableOp keys on the exact row count, so a segment of any other length fell back to the default heuristic -- 202 ms for 1806 frames
# against 196 ms for 2322 (tools/s2mel_scaling.py).  The winning solutions are Tensile kernels without a size-multiple requirement on
# the row dimension (`AF0EM1_AF1EM1` in their names): the same solution serves every row count, so the entries are re-keyed per length.
_TUNED_T0, _TUNED_TH0 = 2322, 1909
_tuned_lengths = set()


def extend_tuned_gemms(T, Th, path=TUNED_GEMMS):
    """Re-key the recorded winners of the DiT / WaveNet GEMMs (rows 2T, T, 2Th, 2Th + 4, Th at the recorded length) to this segment's
    row counts and hand them to TunableOp.  Once per distinct (T, Th); no-op when the results file was not taken."""
    if (T, Th) in _tuned_lengths or (T, Th) == (_TUNED_T0, _TUNED_TH0):
        return False
    _tuned_lengths.add((T, Th))
    import tempfile

    import torch.cuda.tunable as tn

    sub = {str(2 * _TUNED_T0): str(2 * T), str(_TUNED_T0): str(T), str(_TUNED_TH0): str(Th), str(2 * _TUNED_TH0): str(2 * Th),
           str(2 * _TUNED_TH0 + 4): str(2 * Th + 4)}
    head, rows = [], []
    for line in open(path).read().splitlines():
        f = line.split(",")
        if f[0] == "Validator":
            head.append(line)
        elif len(f) >= 4 and f[2] != "Default" and f[0].endswith("_TN"):
            # TN only: both operands K-contiguous with fixed leading dimensions, the row count is a plain free index.  In the TT
            # entries the frame count is a leading dimension and the vectorised one: their solutions carry an alignment requirement
            # (an odd T returned garbage through a re-keyed TT entry -- TunableOp does not look at the library's status)
            toks = f[1].split("_")
            if any(t in sub for t in toks):
                rows.append(",".join([f[0], "_".join(sub.get(t, t) for t in toks)] + f[2:]))
    if not rows:
        return False
    with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as fh:
        fh.write("\n".join(head + rows) + "\n")
    try:
        return bool(tn.read_file(fh.name))
    except Exception:
        return False
    finally:
        os.unlink(fh.name)


class S2Mel:
    def __init__(self, W, cfg=S2MEL_CFG, device="cpu", dtype=torch.float32):
        """dtype: torch.float64 on the CPU gives the high-precision twin of the stage (tests/test_s2mel_twin.py): every weight,
        activation and accumulator in fp64.  What the fp32 path computes before it touches activations -- the folded weights, `t_span`
        and the running t, `t_freqs`, the sinusoid arguments 1000 t f with their cos / sin, the RoPE table -- is the model's definition:
        the twin computes those in fp32 exactly as the default does and widens them, so it differs from fp32 by rounding alone."""
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        self.dtype = dtype
        if dtype not in (torch.float32, torch.float64) or (self.device.type == "cuda" and dtype != torch.float32):
            raise ValueError(f"S2Mel: dtype {dtype} on {self.device} (fp32 anywhere; fp64 on the CPU leg only: the HIP kernels are fp32)")
        self.tuned_gemms = False
        if self.device.type == "cuda" and os.environ.get("IXTTS_NO_TUNED_GEMMS") != "1":
            self.tuned_gemms = use_tuned_gemms()
        W = fold_weight_norm(dict(W))
        self.W = {k: v.to(self.device, torch.float32).to(dtype) for k, v in W.items()}
        H = cfg["hidden_dim"]
        self.head_dim = H // cfg["num_heads"]
        half = 128
        self.t_freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half).to(self.device).to(dtype)
        self._rope = None
        self._t_consts = {}  # (n_timesteps, step, batch), name -> what a DiT evaluation derives from t alone (`_t_const`)
        # derived weights (exact re-arrangements: concatenations / column splits of the reference's matrices)
        W, C_, L = self.W, cfg["in_channels"], cfg["depth"]
        t = "cfm.estimator.transformer."
        self.w13 = [torch.cat([W[t + f"layers.{i}.feed_forward.w1.weight"], W[t + f"layers.{i}.feed_forward.w3.weight"]], 0).contiguous() for i in range(L)]
        self.skip_w = {i: (W[t + f"layers.{i}.skip_in_linear.weight"][:, :H].contiguous(), W[t + f"layers.{i}.skip_in_linear.weight"][:, H:].contiguous())
                       for i in range(L // 2 + 1, L)}
        names = [t + f"layers.{i}.{n}" for i in range(L) for n in ("attention_norm", "ffn_norm")] + [t + "norm"]
        self.proj_w = torch.cat([W[n + ".project_layer.weight"] for n in names], 0).contiguous()  # every AdaLN projection of a step: one GEMM
        self.proj_b = torch.cat([W[n + ".project_layer.bias"] for n in names], 0).contiguous()
        mw = W["cfm.estimator.cond_x_merge_linear.weight"]  # input = [x (C) | prompt_x (C) | cond (H) | style]
        self.merge_x, self.merge_rest = mw[:, :C_].contiguous(), mw[:, C_:].contiguous()
        wn = "cfm.estimator.wavenet."
        self.wn_taps = [[W[wn + f"in_layers.{i}.conv.conv.weight"][:, :, j].contiguous() for j in range(cfg["wavenet_kernel"])]
                        for i in range(cfg["wavenet_layers"])]
        # WaveNet with the residual / skip 1x1 convs as in-place accumulating GEMMs: their biases are constants per channel, so
        # the residual ones are carried forward into the next layer's conv bias (a reflect-padded constant stays a constant:
        # conv(x + c) = conv(x) + (sum of taps) c) and the skip ones are added once at the end
        nl, Hw = cfg["wavenet_layers"], cfg["wavenet_hidden"]
        self.wn_r1, self.wn_r2, self.wn_bin = [], [], []
        carry = torch.zeros(Hw, device=self.device, dtype=dtype)
        self.wn_out_bias = torch.zeros(Hw, device=self.device, dtype=dtype)
        for i in range(nl):
            rw, rb = W[wn + f"res_skip_layers.{i}.conv.conv.weight"][:, :, 0], W[wn + f"res_skip_layers.{i}.conv.conv.bias"]
            self.wn_bin.append(W[wn + f"in_layers.{i}.conv.conv.bias"] + sum(self.wn_taps[i]) @ carry)
            if i < nl - 1:
                self.wn_r1.append(rw[:Hw].contiguous())
                self.wn_r2.append(rw[Hw:].contiguous())
                carry = carry + rb[:Hw]
                self.wn_out_bias = self.wn_out_bias + rb[Hw:]
            else:
                self.wn_r1.append(None)
                self.wn_r2.append(rw.contiguous())
                self.wn_out_bias = self.wn_out_bias + rb
        sw = W["cfm.estimator.skip_linear.weight"]  # input = [x_res (H) | x (C)]
        self.skipl_res, self.skipl_x = sw[:, :H].contiguous(), sw[:, H:].contiguous()
        # split-product GEMMs with fused epilogues (csrc/gemm_x6.hip) on the device, packed once here: [w1; w3] with the SwiGLU in its
        # epilogue, and each WaveNet in_layer's k taps as ONE GEMM (K = k x Hw over row-shifted windows of one split) with the gate in
        # its epilogue -- the two halves interleaved in 32-row blocks (gemm.interleave_halves).  The CPU leg keeps torch's GEMMs.
        self.x6_w13, self.x6_wn = None, None
        if self.device.type == "cuda" and H % 64 == 0:
            inter = self.w13[0].shape[0] // 2
            self.x6_w13 = [G.PackedLinear(G.interleave_halves(w[:inter], w[inter:])) for w in self.w13]
            self.x6_wn = [G.PackedLinear(G.interleave_halves(torch.cat(tp, 1)[:Hw], torch.cat(tp, 1)[Hw:]), G.interleave_halves(b[:Hw], b[Hw:]))
                          for tp, b in zip(self.wn_taps, self.wn_bin)]

    def _x6(self, packs):
        """Whether the device GEMMs with fused epilogues are taken (`IXTTS_S2MEL_GEMM=library`: torch's library GEMMs, for A/B)."""
        return packs is not None and os.environ.get("IXTTS_S2MEL_GEMM", "x6") != "library"

    # ------------------------------------------------------------------ small pieces
    def gpt_layer(self, latent):
        x = _lin(latent, self.W, "gpt_layer.0")
        x = _lin(x, self.W, "gpt_layer.1")
        return _lin(x, self.W, "gpt_layer.2")

    def vq2emb(self, codes):
        """codes [B, n] -> [B, n, semantic_dim] (FactorizedVectorQuantize.vq2emb, then the pipeline's transpose)."""
        emb = self.W["quantizer.codebook.weight"][codes.long()]  # [B,n,8]
        out = conv1d(emb.transpose(1, 2), self.W["quantizer.out_project.weight"], self.W["quantizer.out_project.bias"])
        return out.transpose(1, 2)

    def length_regulator(self, x, ylens):
        """InterpolateRegulator.forward, continuous input: x [B, n, in] -> [B, max(ylens), C] (masked)."""
        W = self.W
        x = _lin(x, W, "length_regulator.content_in_proj")
        T = int(ylens.max())
        x = x.transpose(1, 2).contiguous()
        if x.dtype == torch.float32:
            x = F.interpolate(x, size=T, mode="nearest")
        else:  # the fp32 op's choice of source frames (its index arithmetic runs in the tensor's precision): the model's definition
            src = F.interpolate(torch.arange(x.shape[-1], dtype=torch.float32)[None, None], size=T, mode="nearest")[0, 0].long()
            x = x[..., src.to(x.device)]
        for i in range(self.cfg["lr_n_blocks"]):
            x = conv1d(x, W[f"length_regulator.model.{3 * i}.weight"], W[f"length_regulator.model.{3 * i}.bias"], padding=1)
            x = F.group_norm(x, 1, W[f"length_regulator.model.{3 * i + 1}.weight"], W[f"length_regulator.model.{3 * i + 1}.bias"], 1e-5)
            x = F.mish(x)
        n = 3 * self.cfg["lr_n_blocks"]
        x = conv1d(x, W[f"length_regulator.model.{n}.weight"], W[f"length_regulator.model.{n}.bias"])
        mask = (torch.arange(T, device=x.device).unsqueeze(0) < ylens.unsqueeze(1)).unsqueeze(-1)
        return x.transpose(1, 2) * mask

    def _t_embed(self, t, prefix):
        args = 1000.0 * t[:, None].float() * self.t_freqs[None].float()  # fp32 arguments, cos and sin whatever self.dtype is
        emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1).to(self.dtype)
        h = F.silu(_lin(emb, self.W, prefix + ".mlp.0"))
        return _lin(h, self.W, prefix + ".mlp.2")

    def _t_const(self, tkey, name, fn):
        """`fn()`, computed once per (tkey, name): the pieces of a DiT evaluation that depend on the Euler step's t alone -- the two
        timestep embeddings, the AdaLN (weight | bias) slabs, the WaveNet's cond_layer output, the final layer's (shift | scale).
        t_span = linspace(0, 1, n + 1) does not depend on the request, so they are constants of tkey = (n_timesteps, step, batch) for
        this model's weights, device and dtype: the same calls on the same inputs, made once (25 steps x ~0.3 MB at production width).
        Consumers only read them.  tkey None, or IXTTS_S2MEL_TCACHE=0: computed every time."""
        if tkey is None or os.environ.get("IXTTS_S2MEL_TCACHE", "1") == "0":
            return fn()
        v = self._t_consts.get((tkey, name))
        if v is None:
            v = self._t_consts[(tkey, name)] = fn()
        return v

    def _rope_cache(self, T):
        if self._rope is None or self._rope.shape[0] < T:
            n = self.head_dim
            freqs = 1.0 / (10000.0 ** (torch.arange(0, n, 2)[: n // 2].float() / n))
            ang = torch.outer(torch.arange(max(T, 64)).float(), freqs)
            self._rope = torch.polar(torch.ones_like(ang), ang).to(self.device)  # complex64 [T, d/2]
            if self.dtype == torch.float64:
                self._rope = self._rope.to(torch.complex128)  # the fp32 table, widened
        return self._rope[:T]

    @staticmethod
    def _rotary(x, fc):
        """apply_rotary_emb (gpt_fast/model.py:348-360): (x0 + i x1) * (cos + i sin) on interleaved pairs, as one
        complex multiply.  x [B,T,h,d] fp32, fc complex [T,d/2]."""
        xc = torch.view_as_complex(x.reshape(*x.shape[:-1], -1, 2))
        return torch.view_as_real(xc * fc.view(1, fc.shape[0], 1, fc.shape[1])).flatten(3)

    def _attention(self, qkv, B, T, mask):
        """RoPE on q, k + softmax(q k^T / sqrt(d)) v (gpt_fast/model.py:289-312).  qkv [B*T, 3H] -> [B*T, H]."""
        H, nh, hd = self.cfg["hidden_dim"], self.cfg["num_heads"], self.head_dim
        fc = self._rope_cache(T)
        if mask is None and hd == 64 and qkv.is_cuda:
            v4 = qkv.view(B, T, 3, nh, hd)
            if G.fused() and fc.dtype == torch.complex64 and os.environ.get("IXTTS_ATTN_FULL", "x3") != "f32":
                # the flash kernel on strided views of the GEMM output rotates q and k as it splits them: no rotation pass, no copies
                return attn_full(v4[:, :, 0], v4[:, :, 1], v4[:, :, 2], rope=fc).reshape(B * T, H)
            # in-place rotation on the GEMM output, then the flash kernel on strided views of it
            with torch.cuda.device(qkv.device):
                _hip_call("ixtts_rope_qk_f32", qkv.data_ptr(), torch.view_as_real(fc).data_ptr(), B, T, H, hd)
            return attn_full(v4[:, :, 0], v4[:, :, 1], v4[:, :, 2]).reshape(B * T, H)
        q, k, v = qkv.view(B, T, 3 * H).split([H, H, H], dim=-1)
        q = self._rotary(q.reshape(B, T, nh, hd), fc)
        k = self._rotary(k.reshape(B, T, nh, hd), fc)
        v = v.reshape(B, T, nh, hd)
        y = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=mask, dropout_p=0.0)
        return y.transpose(1, 2).reshape(B * T, H)

    def _transformer(self, x, c, mask, tkey=None):
        """Transformer.forward with U-ViT skips (gpt_fast/model.py:167-207): x [B,T,H], c [B,H] -> [B,T,H].  Residual adds
        ride in the GEMM epilogues (addmm), [w1; w3] is one GEMM, the skip concat is two accumulated GEMMs."""
        W, cfg = self.W, self.cfg
        B, T, H = x.shape
        L = cfg["depth"]
        # (weight | bias) of every AdaLN, one contiguous [B, 2H] slab per norm
        wb_all = self._t_const(tkey, "wb_all", lambda: F.linear(c, self.proj_w, self.proj_b).view(B, 2 * L + 1, 2 * H).transpose(0, 1).contiguous())
        x = x.reshape(B * T, H)
        x6 = x.is_cuda and self._x6(self.x6_w13)
        fuse = G.fused() and H % 64 == 0 and H <= 1024
        skips = []
        for i in range(L):
            p = f"cfm.estimator.transformer.layers.{i}."
            if i > L // 2:
                wa, wb_ = self.skip_w[i]
                x = F.linear(skips.pop(), wb_, W[p + "skip_in_linear.bias"]).addmm_(x, wa.t())
            a = adaln_rmsnorm(x.view(B, T, H), wb_all[2 * i], W[p + "attention_norm.norm.weight"])
            y = self._attention(F.linear(a.view(B * T, H), W[p + "attention.wqkv.weight"]), B, T, mask)
            # residuals accumulate in place where the input is private (layer inputs 1..L/2 are also the saved U-ViT skips)
            h = torch.addmm(x, y, W[p + "attention.wo.weight"].t()) if 0 < i <= L // 2 else x.addmm_(y, W[p + "attention.wo.weight"].t())
            if x6 and fuse:  # the norm writes the planes [w1; w3] reads
                u = G.pair_linear(adaln_rmsnorm_planes(h.view(B, T, H), wb_all[2 * i + 1], W[p + "ffn_norm.norm.weight"]), self.x6_w13[i], G.SWIGLU)
            else:
                f = adaln_rmsnorm(h.view(B, T, H), wb_all[2 * i + 1], W[p + "ffn_norm.norm.weight"]).view(B * T, H)
                u = G.pair_linear(f, self.x6_w13[i], G.SWIGLU) if x6 else swiglu(F.linear(f, self.w13[i]))
            x = h.addmm_(u, W[p + "feed_forward.w2.weight"].t())
            if i < L // 2:
                skips.append(x)
        return adaln_rmsnorm(x.view(B, T, H), wb_all[2 * L], W["cfm.estimator.transformer.norm.norm.weight"])

    def _wavenet(self, x, x_mask, g, full):
        """WN.forward: reflect-padded dilated convs, tanh*sigmoid gate, residual/skip split (wavenet.py:142-167).
        x [B,Hw,T]; g [B,Hw] (timestep embedding); `full`: every sequence spans T, so the mask multiplies are identities."""
        W, cfg = self.W, self.cfg
        Hw, nl, k = cfg["wavenet_hidden"], cfg["wavenet_layers"], cfg["wavenet_kernel"]
        p = "cfm.estimator.wavenet."
        g = F.linear(g, W[p + "cond_layer.conv.conv.weight"][:, :, 0], W[p + "cond_layer.conv.conv.bias"])  # 1x1 conv on a length-1 signal
        out = None
        for i in range(nl):
            d = cfg["wavenet_dilation_rate"] ** i
            tot = (k - 1) * d
            right = tot // 2
            xin = _pad_reflect(x, tot - right, right)  # SConv1d non-causal: left = total - total//2 (encodec.py:224-227)
            if x.is_cuda:
                # k accumulated GEMMs on shifted views of the padded input (one per tap) instead of im2col + GEMM
                wk, T_ = self.wn_taps[i], x.shape[-1]
                acc = W[p + f"in_layers.{i}.conv.conv.bias"][None, :, None].expand(x.shape[0], -1, T_)
                for j in range(k):  # the first tap materialises bias + W_0 x, the others accumulate in place (no copies)
                    wj, xj = wk[j].expand(x.shape[0], -1, -1), xin[:, :, j * d:j * d + T_]
                    acc = torch.baddbmm(acc, wj, xj) if j == 0 else acc.baddbmm_(wj, xj)
                xin = acc
            else:
                xin = conv1d(xin, W[p + f"in_layers.{i}.conv.conv.weight"], W[p + f"in_layers.{i}.conv.conv.bias"], dilation=d)
            acts = wn_gate(xin, g, i * 2 * Hw, Hw)
            rs = conv1d(acts, W[p + f"res_skip_layers.{i}.conv.conv.weight"], W[p + f"res_skip_layers.{i}.conv.conv.bias"])
            if i < nl - 1:
                x = x + rs[:, :Hw]
                if not full:
                    x = x * x_mask
                out = rs[:, Hw:] if out is None else out + rs[:, Hw:]
            else:
                out = rs if out is None else out + rs
        return out if full else out * x_mask

    def _wavenet_gemm(self, x, g):
        """The same network for the pipeline's case (GPU, every sequence spans T): every conv is an accumulating batched GEMM,
        no element-wise adds in between (see __init__); returns the skip sum WITHOUT `wn_out_bias` (the caller's linear adds it)."""
        W, cfg = self.W, self.cfg
        Hw, nl, k = cfg["wavenet_hidden"], cfg["wavenet_layers"], cfg["wavenet_kernel"]
        B, _, T_ = x.shape
        p = "cfm.estimator.wavenet."
        g = F.linear(g, W[p + "cond_layer.conv.conv.weight"][:, :, 0], W[p + "cond_layer.conv.conv.bias"])
        x = x.contiguous()
        out = None
        for i in range(nl):
            d = cfg["wavenet_dilation_rate"] ** i
            tot = (k - 1) * d
            right = tot // 2
            xin = _pad_reflect(x, tot - right, right)
            acc = self.wn_bin[i][None, :, None].expand(B, -1, T_)
            for j in range(k):
                wj, xj = self.wn_taps[i][j].expand(B, -1, -1), xin[:, :, j * d:j * d + T_]
                acc = torch.baddbmm(acc, wj, xj) if j == 0 else acc.baddbmm_(wj, xj)
            acts = wn_gate(acc, g, i * 2 * Hw, Hw)
            if i < nl - 1:
                x = x.baddbmm_(self.wn_r1[i].expand(B, -1, -1), acts)
            r2 = self.wn_r2[i].expand(B, -1, -1)
            out = torch.bmm(r2, acts) if out is None else out.baddbmm_(r2, acts)
        return out

    def _wavenet_rows(self, h, g, tkey=None):
        """The same network with sequences as ROWS (h [B,T,C], dilation 1): every conv is a row-major GEMM `X W^T` (the
        library's fast layout; the channel-major form above runs them at 0.6x the rate).  The B sequences sit in one
        reflect-padded buffer [B, T+k-1, C]; tap j of the k-tap conv is that buffer, flattened, shifted by j rows, so ONE
        GEMM per tap covers all sequences -- the k-1 rows that straddle two sequences are computed and never read (their
        residual update lands in padding rows, which are refreshed before the next layer reads them -- or, on the split-product GEMM,
        never read: its split takes each padding row from the interior row it mirrors).
        Returns the skip sum [B,T,C] (a strided view) WITHOUT `wn_out_bias`."""
        W, cfg = self.W, self.cfg
        Hw, nl, k = cfg["wavenet_hidden"], cfg["wavenet_layers"], cfg["wavenet_kernel"]
        assert cfg["wavenet_dilation_rate"] == 1
        B, T_, _ = h.shape
        p = "cfm.estimator.wavenet."
        g = self._t_const(tkey, "wn_cond", lambda: F.linear(g, W[p + "cond_layer.conv.conv.weight"][:, :, 0], W[p + "cond_layer.conv.conv.bias"]))
        tot = k - 1
        right = tot // 2
        left = tot - right
        Tp = T_ + tot
        P = torch.empty(B, Tp, Hw, device=h.device, dtype=h.dtype)
        P[:, left:left + T_] = h
        P2 = P.view(B * Tp, Hw)
        M = B * Tp - tot
        centre = P2[left:left + M]  # the input row under output row r
        out = torch.empty(B * Tp, Hw, device=h.device, dtype=h.dtype)
        x6 = self._x6(self.x6_wn)
        fuse = G.fused()
        for i in range(nl):
            if x6:  # the k taps + bias + gate: one GEMM over one split of the padded rows, which reads halo rows from their mirror rows
                if not fuse:
                    reflect_halo_rows(P, T_, left, right)
                acts = G.pair_linear(G.split(P2, halo=(T_, left, right) if fuse else None), self.x6_wn[i], G.GATE, taps=k, gate=g, gate_off=i * 2 * Hw,
                                     rows_per_batch=Tp)
            else:
                reflect_halo_rows(P, T_, left, right)
                acc = torch.addmm(self.wn_bin[i], P2[:M], self.wn_taps[i][0].t())
                for j in range(1, k):
                    acc.addmm_(P2[j:j + M], self.wn_taps[i][j].t())
                acts = wn_gate_rows(acc, g, i * 2 * Hw, Hw, Tp)
            if i < nl - 1:
                centre.addmm_(acts, self.wn_r1[i].t())
            if i == 0:
                torch.mm(acts, self.wn_r2[i].t(), out=out[:M])
            else:
                out[:M].addmm_(acts, self.wn_r2[i].t())
        return out.view(B, Tp, Hw)[:, :T_]

    # ------------------------------------------------------------------ DiT + CFM
    def dit_prepare(self, prompt_x, x_lens, style, cond):
        """Everything of DiT.forward that does not depend on (x, t): computed once per CFM solve instead of once per
        Euler step.  prompt_x [B,80,T]; cond [B,T,content]; style [B,style_dim]."""
        W = self.W
        e = "cfm.estimator."
        B, _, T = prompt_x.shape
        cond = _lin(cond, W, e + "cond_projection")
        rest = torch.cat([prompt_x.transpose(1, 2), cond, style[:, None, :].expand(B, T, style.shape[-1])], dim=-1)
        base = F.linear(rest, self.merge_rest, W[e + "cond_x_merge_linear.bias"])  # cond_x_merge_linear minus its x columns
        x_mask = (torch.arange(T, device=prompt_x.device).unsqueeze(0) < x_lens.unsqueeze(1)).unsqueeze(1)  # [B,1,T]
        full = int(x_lens.min()) >= T
        if full:
            attn_mask = None  # the pipeline always runs one full-length sequence: an all-true key mask is no mask
        else:
            attn_mask = x_mask[:, None, :].expand(x_mask.shape[0], 1, T, T)
            if attn_mask.shape[0] != B:
                attn_mask = attn_mask.expand(B, 1, T, T)
        return dict(B=B, T=T, base=base, x_mask=x_mask.to(base.dtype), attn_mask=attn_mask, full=full)

    def dit_step(self, ctx, x, t, out_from=0, tkey=None):
        """The (x, t)-dependent part of DiT.forward (diffusion_transformer.py:186-257).  x [B,80,T] or [1,80,T] shared by
        the whole batch (the CFG stack feeds the same x to both branches); t [B].

        out_from > 0: the caller only uses frames [out_from, T) of the result (the CFM solver zeroes the prompt frames of x
        after every step).  After the transformer nothing mixes frames except the WaveNet's k-tap convs, so the head runs on
        frames [out_from - halo, T) only, halo = the WaveNet's receptive field; the returned tensor covers [out_from, T) and
        equals the full computation there.

        tkey: names t among the values the solver visits (`_t_const`); what depends on t alone is then computed once per model."""
        W, cfg = self.W, self.cfg
        e = "cfm.estimator."
        B, T, base = ctx["B"], ctx["T"], ctx["base"]
        xt = x.transpose(1, 2)  # [Bx,T,80]
        if tkey is not None:
            tkey = tuple(tkey) + (int(t.shape[0]),)
        t1 = self._t_const(tkey, "t1", lambda: self._t_embed(t, e + "t_embedder"))
        x_in = base + F.linear(xt, self.merge_x)  # broadcasts a shared x over the batch
        x_res = self._transformer(x_in, t1, ctx["attn_mask"], tkey)
        halo = sum((cfg["wavenet_kernel"] - 1) * cfg["wavenet_dilation_rate"] ** i for i in range(cfg["wavenet_layers"])) // 2 + 1
        lo = max(0, out_from - halo) if (ctx["full"] and out_from > 0) else 0
        if lo > 0:
            x_res, xt = x_res[:, lo:], xt[:, lo:]
        Th = T - lo
        if self.tuned_gemms and os.environ.get("IXTTS_TUNED_ANY_LENGTH", "1") == "1":
            extend_tuned_gemms(T, Th)
        x_res = F.linear(x_res, self.skipl_res, W[e + "skip_linear.bias"]) + F.linear(xt, self.skipl_x)
        h = _lin(x_res, W, e + "conv1")
        t2 = self._t_const(tkey, "t2", lambda: self._t_embed(t, e + "t_embedder2"))
        gemm_form = h.is_cuda and ctx["full"] and Th > 2 * cfg["wavenet_kernel"] * cfg["wavenet_dilation_rate"] ** (cfg["wavenet_layers"] - 1)
        if gemm_form and cfg["wavenet_dilation_rate"] == 1:
            h = self._wavenet_rows(h, t2, tkey) + F.linear(x_res, W[e + "res_projection.weight"], W[e + "res_projection.bias"] + self.wn_out_bias)
        elif gemm_form:
            h = self._wavenet_gemm(h.transpose(1, 2), t2).transpose(1, 2) + F.linear(x_res, W[e + "res_projection.weight"],
                                                                                     W[e + "res_projection.bias"] + self.wn_out_bias)
        else:
            mask = ctx["x_mask"][:, :, lo:] if lo > 0 else ctx["x_mask"]
            h = self._wavenet(h.transpose(1, 2), mask, t2, ctx["full"]).transpose(1, 2) + _lin(x_res, W, e + "res_projection")
        ss = self._t_const(tkey, "final_ss", lambda: _lin(F.silu(t1), W, e + "final_layer.adaLN_modulation.1"))
        h = ln_modulate(h, ss)
        h = _lin(h, W, e + "final_layer.linear").transpose(1, 2)
        out = conv1d(h, W[e + "conv2.weight"], W[e + "conv2.bias"])
        return out[:, :, out_from - lo:] if out_from > 0 else out

    def dit(self, x, prompt_x, x_lens, t, style, cond):
        """DiT.forward, eval mode.  x, prompt_x [B,80,T]; cond [B,T,content]."""
        return self.dit_step(self.dit_prepare(prompt_x, x_lens, style, cond), x, t)

    @torch.no_grad()
    def cfm_inference(self, mu, x_lens, prompt, style, n_timesteps=25, inference_cfg_rate=0.7, noise=None, temperature=1.0):
        """BASECFM.inference + solve_euler (flow_matching.py:30-115).  mu [B,T,content]; prompt [B,80,Tp]; noise [B,80,T]."""
        B, T = mu.shape[0], mu.shape[1]
        assert B == 1, "CFM inference is batch-1 (as the reference)"
        z = (torch.randn(B, self.cfg["in_channels"], T, device=mu.device) if noise is None else noise.to(mu.device, torch.float32)).to(self.dtype) * temperature
        t_span = torch.linspace(0, 1, n_timesteps + 1, device=mu.device)
        x = z.clone()
        Tp = prompt.shape[-1]
        prompt_x = torch.zeros_like(x)
        prompt_x[..., :Tp] = prompt[..., :Tp]
        x[..., :Tp] = 0
        if inference_cfg_rate > 0:
            # batch-2 stacking of the conditional and the null branch (the reference supports B == 1 only:
            # its stacked_t has 2 entries whatever B is, flow_matching.py:88-93); x is shared by the two
            ctx = self.dit_prepare(torch.cat([prompt_x, torch.zeros_like(prompt_x)], 0), x_lens, torch.cat([style, torch.zeros_like(style)], 0),
                                   torch.cat([mu, torch.zeros_like(mu)], 0))
        else:
            ctx = self.dit_prepare(prompt_x, x_lens, style, mu)
        t = t_span[0]
        # the prompt frames of x are reset to zero after every step (flow_matching.py:112): the velocity there is never used
        skip = Tp if ctx["full"] else 0
        for step in range(1, len(t_span)):
            dt = t_span[step] - t_span[step - 1]
            if inference_cfg_rate > 0:
                d = self.dit_step(ctx, x, torch.stack([t, t]), out_from=skip, tkey=(n_timesteps, step))
                dphi = (1.0 + inference_cfg_rate) * d[0:1] - inference_cfg_rate * d[1:2]
            else:
                dphi = self.dit_step(ctx, x, t.expand(B), out_from=skip, tkey=(n_timesteps, step))
            if skip > 0:
                x[:, :, skip:] += dt * dphi
            else:
                x = x + dt * dphi
            t = t + dt
            x[:, :, :Tp] = 0
        return x

    # ------------------------------------------------------------------ the stage as infer_v2.py:713-731 calls it
    @torch.no_grad()
    def __call__(self, latent, codes, code_lens, prompt_condition, ref_mel, style, n_timesteps=25, inference_cfg_rate=0.7, noise=None, frames=None):
        """`frames` (an int >= 1): the regulator stretches the codes to this many mel frames instead of `target_frames(code_lens)` --
        the speaking rate (`target_frames(n, speed)`) or a fitted duration; the CFM noise is then [1, 80, Tp + frames]."""
        lat = self.gpt_layer(latent)
        S = self.vq2emb(codes) + lat
        target = target_frames(code_lens) if frames is None else torch.tensor([int(frames)], device=code_lens.device)
        cond = self.length_regulator(S, target)
        cat = torch.cat([prompt_condition, cond], dim=1)
        lens = torch.tensor([cat.shape[1]], device=cat.device, dtype=torch.long)
        mel = self.cfm_inference(cat, lens, ref_mel, style, n_timesteps, inference_cfg_rate, noise)
        return mel[:, :, ref_mel.shape[-1]:]

    # ------------------------------------------------------------------ many segments through ONE CFM solve (packed rows)
    def _attention_packed(self, qkv, pk):
        """`_attention` over a pack (qkv [rows, 3H] -> [rows, H]): one varlen HIP attention on the device; per sequence on slices where
        its limits are not met (head_dim != 64, IXTTS_ATTN_FULL=f32) -- the single-sequence path, same result."""
        H, nh, hd = self.cfg["hidden_dim"], self.cfg["num_heads"], self.head_dim
        if qkv.is_cuda and hd == 64 and os.environ.get("IXTTS_ATTN_FULL", "x3") != "f32":
            fc = self._rope_cache(max(pk.lens))
            v4 = qkv.view(pk.rows, 3, nh, hd)
            if G.fused() and fc.dtype == torch.complex64:
                return attn_full_packed(v4[:, 0], v4[:, 1], v4[:, 2], pk, rope=fc).view(pk.rows, H)
            rope_qk_packed(qkv, fc, pk, hd)
            return attn_full_packed(v4[:, 0], v4[:, 1], v4[:, 2], pk).view(pk.rows, H)
        out = torch.empty(pk.rows, H, device=qkv.device, dtype=qkv.dtype)
        if qkv.is_cuda:
            for s in range(pk.n):
                a, b = pk.span(s)
                out[a:b] = self._attention(qkv[a:b], 1, b - a, None)
            return out
        qk = rope_qk_packed(qkv, self._rope_cache(max(pk.lens)), pk, hd)  # the torch form of the device pass
        for s in range(pk.n):
            a, b = pk.span(s)
            q, k, v = (qk[a:b, :H], qk[a:b, H:2 * H], qkv[a:b, 2 * H:])
            y = F.scaled_dot_product_attention(*(z.reshape(1, b - a, nh, hd).transpose(1, 2) for z in (q, k, v)), dropout_p=0.0)
            out[a:b] = y.transpose(1, 2).reshape(b - a, H)
        return out

    def _transformer_packed(self, x, c, pk):
        """`_transformer` over a pack: x [rows, H], c [n, H] (one timestep embedding per sequence)."""
        W, cfg = self.W, self.cfg
        H, L = cfg["hidden_dim"], cfg["depth"]
        wb_all = F.linear(c, self.proj_w, self.proj_b).view(pk.n, 2 * L + 1, 2 * H).transpose(0, 1).contiguous()
        x6 = x.is_cuda and self._x6(self.x6_w13)
        fuse = G.fused() and H % 64 == 0 and H <= 1024
        skips = []
        for i in range(L):
            p = f"cfm.estimator.transformer.layers.{i}."
            if i > L // 2:
                wa, wb_ = self.skip_w[i]
                x = F.linear(skips.pop(), wb_, W[p + "skip_in_linear.bias"]).addmm_(x, wa.t())
            a = adaln_rmsnorm_packed(x, wb_all[2 * i], W[p + "attention_norm.norm.weight"], pk)
            y = self._attention_packed(F.linear(a, W[p + "attention.wqkv.weight"]), pk)
            h = torch.addmm(x, y, W[p + "attention.wo.weight"].t()) if 0 < i <= L // 2 else x.addmm_(y, W[p + "attention.wo.weight"].t())
            if x6 and fuse:
                u = G.pair_linear(adaln_rmsnorm_planes(h, wb_all[2 * i + 1], W[p + "ffn_norm.norm.weight"], pk=pk), self.x6_w13[i], G.SWIGLU)
            else:
                f = adaln_rmsnorm_packed(h, wb_all[2 * i + 1], W[p + "ffn_norm.norm.weight"], pk)
                u = G.pair_linear(f, self.x6_w13[i], G.SWIGLU) if x6 else swiglu(F.linear(f, self.w13[i]))
            x = h.addmm_(u, W[p + "feed_forward.w2.weight"].t())
            if i < L // 2:
                skips.append(x)
        return adaln_rmsnorm_packed(x, wb_all[2 * L], W["cfm.estimator.transformer.norm.norm.weight"], pk)

    def _wavenet_packed(self, h, g, hp):
        """`_wavenet_rows` over a pack: h [rows, Hw] (sequences of `hp`), g [n, Hw].  Every sequence sits in one row buffer followed by
        its own k - 1 halo rows (`hp.padded`: the padded offsets), so each tap is still ONE GEMM over all of them.  Returns the skip sum
        [rows, Hw] WITHOUT `wn_out_bias`."""
        W, cfg = self.W, self.cfg
        Hw, nl, k = cfg["wavenet_hidden"], cfg["wavenet_layers"], cfg["wavenet_kernel"]
        assert cfg["wavenet_dilation_rate"] == 1
        p = "cfm.estimator.wavenet."
        g = F.linear(g, W[p + "cond_layer.conv.conv.weight"][:, :, 0], W[p + "cond_layer.conv.conv.bias"])
        tot = k - 1
        right = tot // 2
        left = tot - right
        pp, interior = hp.padded, hp.interior
        P2 = torch.empty(pp.rows, Hw, device=h.device, dtype=h.dtype)
        P2[interior] = h
        M = pp.rows - tot
        centre = P2[left:left + M]
        out = torch.empty(pp.rows, Hw, device=h.device, dtype=h.dtype)
        x6 = h.is_cuda and self._x6(self.x6_wn)
        fuse = G.fused()
        for i in range(nl):
            if x6:
                if not fuse:
                    reflect_halo_rows_packed(P2, pp, left, right)
                acts = G.pair_linear(G.split(P2, halo=(pp, left, right) if fuse else None), self.x6_wn[i], G.GATE, taps=k, gate=g, gate_off=i * 2 * Hw,
                                     seq_off=pp)
            else:
                reflect_halo_rows_packed(P2, pp, left, right)
                acc = torch.addmm(self.wn_bin[i], P2[:M], self.wn_taps[i][0].t())
                for j in range(1, k):
                    acc.addmm_(P2[j:j + M], self.wn_taps[i][j].t())
                acts = wn_gate_rows_packed(acc, g, i * 2 * Hw, Hw, pp)
            if i < nl - 1:
                centre.addmm_(acts, self.wn_r1[i].t())
            if i == 0:
                torch.mm(acts, self.wn_r2[i].t(), out=out[:M])
            else:
                out[:M].addmm_(acts, self.wn_r2[i].t())
        return out[interior - left]

    def _halo(self):
        cfg = self.cfg
        return sum((cfg["wavenet_kernel"] - 1) * cfg["wavenet_dilation_rate"] ** i for i in range(cfg["wavenet_layers"])) // 2 + 1

    def packable(self, T, Tp, device=None):
        """Whether a segment of T frames (Tp of them prompt) can join a packed solve on `device`: on the GPU its WaveNet rows must take
        the row-GEMM form there (more than 2 k frames past the halo, dilation 1) -- a shorter one is solved on its own, as `__call__`."""
        dev = self.device if device is None else torch.device(device)
        if dev.type != "cuda":
            return True
        cfg = self.cfg
        Th = T - max(0, Tp - self._halo())
        return cfg["wavenet_dilation_rate"] == 1 and Th > 2 * cfg["wavenet_kernel"]

    def _cfm_packed(self, segs, n_timesteps, inference_cfg_rate):
        """The Euler solve of `cfm_inference` for several segments at once.  segs: dicts mu [1,T,content], prompt [1,80,Tp'], style
        [1,sd], z [1,80,T].  Sequences (rows of every GEMM and row kernel): all conditional ones, then, with CFG, all null ones; x
        (shared by the two branches) is packed once.  Returns x [1,80,T] per segment."""
        W, cfg = self.W, self.cfg
        e = "cfm.estimator."
        dev = segs[0]["mu"].device
        C_, H = cfg["in_channels"], cfg["hidden_dim"]
        n = len(segs)
        lens = [s["mu"].shape[1] for s in segs]
        Tps = [min(s["prompt"].shape[-1], T) for s, T in zip(segs, lens)]
        R = sum(lens)
        cfg_on = inference_cfg_rate > 0
        nb = 2 if cfg_on else 1
        pk = RowPack(lens * nb, dev)
        xo = pk.off[:n + 1]
        # x rows [R, C]: the noise with the prompt frames zeroed; the velocities of frames >= Tp are the only ones used
        x = torch.cat([s["z"][0].t() for s in segs], 0).contiguous()
        keep = torch.cat([torch.arange(xo[i] + Tps[i], xo[i + 1]) for i in range(n)]).to(dev)
        pmask = torch.ones(R, 1, device=dev, dtype=self.dtype)
        for i in range(n):
            pmask[xo[i]:xo[i] + Tps[i]] = 0
        x.mul_(pmask)
        # dit_prepare: the (x, t)-independent part of the merge linear, per row
        prompt_rows = torch.zeros(R, C_, device=dev, dtype=self.dtype)
        for i, s in enumerate(segs):
            prompt_rows[xo[i]:xo[i] + Tps[i]] = s["prompt"][0, :, :Tps[i]].t()
        mu = torch.cat([s["mu"][0] for s in segs], 0)
        style = torch.cat([s["style"].expand(T, -1) for s, T in zip(segs, lens)], 0)
        rest = torch.cat([prompt_rows, _lin(mu, W, e + "cond_projection"), style], -1)
        if cfg_on:
            rest = torch.cat([rest, torch.cat([torch.zeros_like(prompt_rows), _lin(torch.zeros_like(mu), W, e + "cond_projection"), torch.zeros_like(style)], -1)], 0)
        base = F.linear(rest, self.merge_rest, W[e + "cond_x_merge_linear.bias"])
        # the WaveNet head: frames [lo, T) of each sequence (lo = Tp - halo), each followed by its k - 1 halo rows
        halo, k = self._halo(), cfg["wavenet_kernel"]
        los = [max(0, Tp - halo) for Tp in Tps] * nb
        head_lens = [L - lo for L, lo in zip(pk.lens, los)]
        hp = RowPack(head_lens, dev)
        hp.padded = RowPack([t + k - 1 for t in head_lens], dev)
        right = (k - 1) // 2
        left = k - 1 - right
        hidx = torch.cat([torch.arange(pk.off[s] + los[s], pk.off[s + 1]) for s in range(pk.n)])
        hp.interior = torch.cat([torch.arange(hp.padded.off[s] + left, hp.padded.off[s] + left + head_lens[s]) for s in range(pk.n)]).to(dev)
        hrows = hidx.to(dev)  # transformer row of each head row
        hx = (hidx - torch.tensor(pk.off[:-1]).repeat_interleave(torch.tensor(head_lens)) +
              torch.tensor(xo[:-1] * nb).repeat_interleave(torch.tensor(head_lens))).to(dev)  # x row of each head row
        # velocity rows of frames >= Tp: cond half and null half of the head rows
        hsel = torch.cat([torch.arange(hp.off[s] + Tps[s % n] - los[s], hp.off[s + 1]) for s in range(pk.n)]).to(dev)
        nkeep = keep.numel()
        t_span = torch.linspace(0, 1, n_timesteps + 1, device=dev)
        t = t_span[0]
        for step in range(1, len(t_span)):
            dt = t_span[step] - t_span[step - 1]
            tt = t.expand(pk.n)
            t1 = self._t_embed(tt, e + "t_embedder")
            x_in = (base.view(nb, R, H) + F.linear(x, self.merge_x)).view(nb * R, H)
            x_res = self._transformer_packed(x_in, t1, pk)
            x_res = x_res.index_select(0, hrows)
            xt = x.index_select(0, hx)
            x_res = F.linear(x_res, self.skipl_res, W[e + "skip_linear.bias"]) + F.linear(xt, self.skipl_x)
            h = _lin(x_res, W, e + "conv1")
            t2 = self._t_embed(tt, e + "t_embedder2")
            h = self._wavenet_packed(h, t2, hp) + F.linear(x_res, W[e + "res_projection.weight"], W[e + "res_projection.bias"] + self.wn_out_bias)
            ss = _lin(F.silu(t1), W, e + "final_layer.adaLN_modulation.1")
            h = ln_modulate_packed(h, ss, hp)
            h = _lin(h, W, e + "final_layer.linear")
            d = F.linear(h.index_select(0, hsel), W[e + "conv2.weight"][:, :, 0], W[e + "conv2.bias"])
            dphi = (1.0 + inference_cfg_rate) * d[:nkeep] - inference_cfg_rate * d[nkeep:] if cfg_on else d
            x.index_add_(0, keep, dt * dphi)
            t = t + dt
            x.mul_(pmask)  # the prompt frames back to zero (flow_matching.py:112)
        return [x[xo[i]:xo[i + 1]].t()[None] for i in range(n)]

    @torch.no_grad()
    def solve_many(self, items, n_timesteps=25, inference_cfg_rate=0.7, noises=None, frames=None):
        """`__call__` for several segments: items are (latent, codes, prompt_condition, ref_mel, style) as `__call__` takes them (code
        lengths = codes.shape[1]); returns one mel [1, 80, frames_i] per item, each equal to its own `__call__` up to fp32
        reassociation.  The length regulator runs per item; the CFM solves of all items run as ONE Euler loop over packed rows
        (`_cfm_packed`), at most IXTTS_S2MEL_BATCH_FRAMES frames per pack (larger requests: several packs, grouped by length).  With
        noises None each item's noise is drawn as n successive `__call__`s would draw it (item order, default generator).  `frames`: per
        item None or the frame count its `__call__` would be given."""
        segs = []
        for i, (latent, codes, prompt_condition, ref_mel, style) in enumerate(items):
            code_lens = torch.tensor([codes.shape[-1]], device=codes.device)
            S = self.vq2emb(codes) + self.gpt_layer(latent)
            target = target_frames(code_lens) if frames is None or frames[i] is None else torch.tensor([int(frames[i])], device=codes.device)
            cond = self.length_regulator(S, target)
            mu = torch.cat([prompt_condition, cond], dim=1)
            T = mu.shape[1]
            z = torch.randn(1, self.cfg["in_channels"], T, device=mu.device) if noises is None or noises[i] is None else \
                noises[i].to(mu.device, torch.float32)
            z = z.to(self.dtype)
            segs.append(dict(mu=mu, prompt=ref_mel, style=style, z=z, Tp=ref_mel.shape[-1]))
        xs = [None] * len(segs)
        budget = max(1, int(os.environ.get("IXTTS_S2MEL_BATCH_FRAMES", str(S2MEL_BATCH_FRAMES))))
        order = sorted(range(len(segs)), key=lambda i: segs[i]["mu"].shape[1])
        groups, cur, used = [], [], 0
        for i in order:
            T = segs[i]["mu"].shape[1]
            if not self.packable(T, segs[i]["Tp"], segs[i]["mu"].device):
                groups.append([i])
                continue
            if cur and used + T > budget:
                groups.append(cur)
                cur, used = [], 0
            cur.append(i)
            used += T
        if cur:
            groups.append(cur)
        for grp in groups:
            if len(grp) == 1 and not self.packable(segs[grp[0]]["mu"].shape[1], segs[grp[0]]["Tp"], segs[grp[0]]["mu"].device):
                s = segs[grp[0]]
                lens = torch.tensor([s["mu"].shape[1]], device=s["mu"].device, dtype=torch.long)
                xs[grp[0]] = self.cfm_inference(s["mu"], lens, s["prompt"], s["style"], n_timesteps, inference_cfg_rate, s["z"])
                continue
            for i, x in zip(grp, self._cfm_packed([segs[i] for i in grp], n_timesteps, inference_cfg_rate)):
                xs[i] = x
        return [x[:, :, s["Tp"]:] for x, s in zip(xs, segs)]
