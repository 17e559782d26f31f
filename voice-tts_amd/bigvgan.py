"""Seam 2: BigVGAN-v2 generator backed by the HIP library.

Mirrors `indextts/s2mel/modules/bigvgan/bigvgan.py:243-400`: constructed from the same
hyper-parameter mapping (`config.json`), fed the same generator state dict (with or
without weight norm), called as `bigvgan(mel_fp32[B,80,F]) -> wav[B,1,256F]`
(`indextts/infer_v2.py:735`).  `remove_weight_norm()` / `eval()` are accepted for
drop-in compatibility (the fold happens once in `load_state_dict`, row V5).
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib
from .weights import BIGVGAN_CFG, fold_weight_norm


# Padded frames (rows x longest row) per batched vocoder pass (`BigVGAN.forward_many`; IXTTS_BV_BATCH_FRAMES).  The workspace grows
# with it: at production width 11 fp32 buffers of 6144 floats per padded frame and 4 plane buffers of 6144 x 6 bytes, 418 KB per
# padded frame -- 1.7 GB at this default (3.4 GB at 8192).  Chosen by tools/bv_batch_perf.py (profiles/bv_batch_perf.json).
BV_BATCH_FRAMES = 4096


def vocoder_batching():
    """The mels of several segments through ONE vocoder pass (`BigVGAN.forward_many`) in `infer_many` and after a packed solve in
    `infer`.  On by default (every row is bit-identical to its own `forward`); IXTTS_BV_BATCH=0: one pass per segment."""
    return os.environ.get("IXTTS_BV_BATCH", "1") != "0"


def vocoder_batch_frames():
    return max(1, int(os.environ.get("IXTTS_BV_BATCH_FRAMES", str(BV_BATCH_FRAMES))))


def plan_vocoder_batches(frames, cap):
    """Groups of row indices for the batched vocoder pass: rows sorted by length (ties in input order), cut greedily so that a group's
    padded size, rows x longest row, stays within `cap` frames; a single row longer than `cap` is a group of its own.  Every index
    appears in exactly one group."""
    order = sorted(range(len(frames)), key=lambda i: (int(frames[i]), i))
    groups, cur = [], []
    for i in order:
        # (sorted ascending: the row being added is the longest of its group)
        if cur and (len(cur) + 1) * int(frames[i]) > cap:
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    return groups


class BigVGAN(nn.Module):
    def __init__(self, h=None, use_cuda_kernel=True, max_frames=4096, fast_sin=False, device=None):
        super().__init__()
        h = dict(BIGVGAN_CFG if h is None else h)
        if not use_cuda_kernel:
            raise RuntimeError("this BigVGAN only has the HIP path (use_cuda_kernel=True); there is no torch fallback")
        if h.get("resblock", "1") != "1" or h.get("activation", "snakebeta") != "snakebeta" or not h.get("snake_logscale", True):
            raise NotImplementedError("HIP BigVGAN implements the shipped config: AMPBlock1 + log-scale SnakeBeta (config.json:9,20-21)")
        if h.get("use_tanh_at_final", False) or h.get("use_bias_at_final", False):
            raise NotImplementedError("HIP BigVGAN implements use_tanh_at_final=false / use_bias_at_final=false (config.json:17-18)")
        self.h = h
        self.device_ = torch.device(device if device is not None else "cuda:0")
        cfg = _lib.BigVGANCfg()
        cfg.num_mels = h["num_mels"]
        cfg.upsample_initial_channel = h["upsample_initial_channel"]
        rates, ks = list(h["upsample_rates"]), list(h["upsample_kernel_sizes"])
        cfg.n_stages = len(rates)
        for i, (u, k) in enumerate(zip(rates, ks)):
            cfg.upsample_rates[i] = u
            cfg.upsample_kernel_sizes[i] = k
        rk, rd = list(h["resblock_kernel_sizes"]), list(h["resblock_dilation_sizes"])
        cfg.n_resblock_kernels = len(rk)
        for j, (k, d) in enumerate(zip(rk, rd)):
            cfg.resblock_kernel_sizes[j] = k
            for m in range(3):
                cfg.resblock_dilations[j][m] = d[m]
        cfg.max_frames = max_frames
        cfg.fast_sin = int(bool(fast_sin))
        self._cfg = cfg
        self.total_up = 1
        for u in rates:
            self.total_up *= u
        self._h = C.c_void_p()
        with torch.cuda.device(self.device_):
            _lib.check(_lib.lib().ixtts_bigvgan_create(C.byref(self._h), C.byref(cfg)), "ixtts_bigvgan_create")
        self._loaded = False

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd, strict=True):
        sd = fold_weight_norm({k: v for k, v in sd.items() if not k.endswith("filter")})
        L = _lib.lib()
        with torch.cuda.device(self.device_):
            for name, t in sd.items():
                t = t.detach().to("cpu", torch.float32).contiguous()
                shape = (C.c_int64 * t.dim())(*t.shape)
                rc = L.ixtts_bigvgan_set_tensor(self._h, name.encode(), t.data_ptr(), shape, t.dim())
                if rc == -5 and not strict:
                    continue
                _lib.check(rc, f"ixtts_bigvgan_set_tensor({name})")
            _lib.check(L.ixtts_bigvgan_finalize(self._h), "ixtts_bigvgan_finalize")
        self._loaded = True
        return self

    def arena(self):
        """(device pointer, bytes) of the packed weight arena -- for the RCCL broadcast at load."""
        p, n = C.c_void_p(), C.c_size_t()
        _lib.check(_lib.lib().ixtts_bigvgan_arena(self._h, C.byref(p), C.byref(n)), "ixtts_bigvgan_arena")
        return p.value, n.value

    def adopt_arena(self):
        with torch.cuda.device(self.device_):
            _lib.check(_lib.lib().ixtts_bigvgan_adopt_arena(self._h), "ixtts_bigvgan_adopt_arena")
        self._loaded = True

    def remove_weight_norm(self):
        return self

    # slots of ixtts_bigvgan_tile_launches: the tiles chosen by score (the names IXTTS_BV_TILE takes), then those a Cout fixes
    TILE_NAMES = {0: ("128x128", "128x96", "64x128", "fixed 32x128", "fixed 64x128"),
                  1: ("128x128", "64x128", "64x64", "fixed 32x256", "fixed 64x128", "fixed 96x128")}
    SCORED_TILES = 3

    def tile_launches(self):
        """Conv launches of this handle so far by tile shape: {"128x128": n, ..., "fixed 64x128": n}.  The first SCORED_TILES keys are
        the tiles the launcher chooses among by score (or IXTTS_BV_TILE names, read when the handle was created), the "fixed" ones those
        a conv's Cout leaves no choice about.  Host counters; the names depend on the handle's kernels (IXTTS_BV_CONV)."""
        counts, f32 = (C.c_int64 * _lib.BIGVGAN_TILE_SLOTS)(), C.c_int()
        _lib.check(_lib.lib().ixtts_bigvgan_tile_launches(self._h, counts, C.byref(f32)), "ixtts_bigvgan_tile_launches")
        return {name: int(counts[i]) for i, name in enumerate(self.TILE_NAMES[f32.value])}

    def flops(self, B, F):
        return _lib.lib().ixtts_bigvgan_flops(self._h, B, F)

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        if not self._loaded:
            raise RuntimeError("BigVGAN: weights not loaded")
        if x.dtype != torch.float32 or not x.is_cuda or x.dim() != 3 or x.shape[1] != self.h["num_mels"]:
            raise RuntimeError(f"BigVGAN.forward expects a CUDA fp32 [B,{self.h['num_mels']},F] mel, got {tuple(x.shape)} {x.dtype} {x.device}")
        x = x.contiguous()
        B, _, F = x.shape
        wav = torch.empty(B, 1, F * self.total_up, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            rc = _lib.lib().ixtts_bigvgan_forward(self._h, x.data_ptr(), B, F, wav.data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "ixtts_bigvgan_forward")
        return wav

    def forward_varlen(self, mel, frames, out=None):
        """One pass over rows of unequal length (`ixtts_bigvgan_forward_varlen`): `mel` fp32 [B, num_mels, Fmax] on the device, row b
        `frames[b] <= Fmax` frames long (the rest is padding and is never read) -> wav [B, 1, Fmax*total_up], zero from
        `frames[b]*total_up` on (`out`: written in place instead, and left as it was from there on).  Row b is bit-identical to
        `forward` on that row alone."""
        if not self._loaded:
            raise RuntimeError("BigVGAN: weights not loaded")
        if mel.dtype != torch.float32 or not mel.is_cuda or mel.dim() != 3 or mel.shape[1] != self.h["num_mels"]:
            raise RuntimeError(f"BigVGAN.forward_varlen expects a CUDA fp32 [B,{self.h['num_mels']},Fmax] mel, got {tuple(mel.shape)} {mel.dtype} {mel.device}")
        mel = mel.contiguous()
        B, _, Fmax = mel.shape
        frames = [int(f) for f in frames]
        if len(frames) != B:
            raise RuntimeError(f"BigVGAN.forward_varlen: {len(frames)} lengths for {B} rows")
        wav = out if out is not None else torch.zeros(B, 1, Fmax * self.total_up, device=mel.device, dtype=torch.float32)
        if wav.shape != (B, 1, Fmax * self.total_up) or wav.dtype != torch.float32 or wav.device != mel.device or not wav.is_contiguous():
            raise RuntimeError(f"BigVGAN.forward_varlen: out must be a contiguous fp32 [{B},1,{Fmax * self.total_up}] tensor on {mel.device}")
        host = (C.c_int * max(B, 1))(*frames)
        with torch.cuda.device(mel.device):
            dev = torch.tensor(frames, dtype=torch.int32, device=mel.device)
            rc = _lib.lib().ixtts_bigvgan_forward_varlen(self._h, mel.data_ptr(), dev.data_ptr(), host, B, Fmax, wav.data_ptr(),
                                                         _lib.current_stream_ptr())
        _lib.check(rc, "ixtts_bigvgan_forward_varlen")
        return wav

    def forward_many(self, mels):
        """Mels of unequal length, fp32 [1, num_mels, F_i] on the device -> [1, 1, F_i*total_up] each, in input order: rows grouped
        by length (`plan_vocoder_batches`, at most IXTTS_BV_BATCH_FRAMES padded frames per group), every group one padded buffer and
        one `forward_varlen` call.  Each result is bit-identical to `forward(mel_i)`."""
        mels = list(mels)
        for m in mels:
            if m.dim() != 3 or m.shape[0] != 1 or m.shape[1] != self.h["num_mels"] or m.dtype != torch.float32 or not m.is_cuda:
                raise RuntimeError(f"BigVGAN.forward_many expects CUDA fp32 [1,{self.h['num_mels']},F] mels, got {tuple(m.shape)} {m.dtype} {m.device}")
        out = [None] * len(mels)
        for group in plan_vocoder_batches([m.shape[2] for m in mels], vocoder_batch_frames()):
            frames = [mels[i].shape[2] for i in group]
            if len(group) == 1:
                out[group[0]] = self.forward(mels[group[0]])
                continue
            pad = torch.zeros(len(group), self.h["num_mels"], max(frames), device=mels[group[0]].device, dtype=torch.float32)
            for b, i in enumerate(group):
                pad[b, :, :frames[b]] = mels[i][0]
            wav = self.forward_varlen(pad, frames)
            for b, i in enumerate(group):
                out[i] = wav[b:b + 1, :, :frames[b] * self.total_up].clone()
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                _lib.lib().ixtts_bigvgan_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass
