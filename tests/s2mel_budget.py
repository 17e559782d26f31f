"""The cases of the s2mel error budget, shared by tests/test_s2mel_twin.py (fp32 CPU leg against the fp64 twin),
tests/test_gpu_s2mel_fp64.py (device paths against the twin) and tools/s2mel_error_budget.py (which records the numbers in
profiles/s2mel_error_budget.json).

Every case is a function of (model, inputs) that runs on whatever leg the model is: `S2Mel(W, cfg)` (fp32, CPU),
`S2Mel(W, cfg, dtype=torch.float64)` (the twin) or `S2Mel(W, cfg, device="cuda:0")`.  Inputs are drawn once in fp32 and widened for
the twin, so all legs see the same numbers; outputs come back as fp64 CPU tensors."""
import contextlib
import os

import torch

import voice_tts_amd.s2mel as S2

CONFIGS = {
    "hd64": lambda: S2.tiny_s2mel_cfg(hidden_dim=128, num_heads=2, wavenet_hidden=128, depth=3),  # head_dim 64: the HIP attention runs
    "prod": lambda: dict(S2.S2MEL_CFG),
}
T, TP = 200, 60                               # frames of the single-segment cases, prompt frames among them
PACK = [(150, 60), (12 + 40, 12), (203, 60)]  # (frames, prompt frames) of the packed solve
T_EVAL, STEPS, CFG_RATE = 0.37, 3, 0.7
SEED = 1234

# device arithmetic modes: environment of each
MODES = {"default": {}, "library_gemm": {"IXTTS_S2MEL_GEMM": "library"}, "attn_f32": {"IXTTS_ATTN_FULL": "f32"}}

CPU_CASES = ("dit_step_window", "cfm3", "packed3")
CASES = ("attention_T150", "attention_T321", "transformer", "wavenet", "dit_step_window", "dit_step_full", "cfm3", "packed3",
         "packed3_vs_segments")


@contextlib.contextmanager
def mode(name):
    old = {k: os.environ.get(k) for m in MODES.values() for k in m}
    try:
        for k in old:
            os.environ.pop(k, None)
        os.environ.update(MODES[name])
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def models(name, device=None):
    """(cfg, fp32 CPU leg, twin[, device model]) from one set of weights."""
    cfg = CONFIGS[name]()
    W = S2.make_s2mel_weights(cfg, seed=SEED)
    out = (cfg, S2.S2Mel(W, cfg), S2.S2Mel(W, cfg, dtype=torch.float64))
    return out + (S2.S2Mel(W, cfg, device=device),) if device is not None else out


def _segment(cfg, g, frames, prompt_frames):
    return dict(mu=torch.randn(1, frames, cfg["content_dim"], generator=g), prompt=torch.randn(1, 80, prompt_frames, generator=g) * 2 - 4,
                style=torch.randn(1, cfg["style_dim"], generator=g), z=torch.randn(1, 80, frames, generator=g))


def inputs(cfg):
    """fp32 inputs of every case, by name."""
    H, Hw = cfg["hidden_dim"], cfg["wavenet_hidden"]
    g = torch.Generator().manual_seed(SEED + 1)
    return dict(
        qkv150=torch.randn(2 * 150, 3 * H, generator=g), qkv321=torch.randn(2 * 321, 3 * H, generator=g),
        tr_x=torch.randn(2, 150, H, generator=g), tr_c=torch.randn(2, H, generator=g),
        wn_h=torch.randn(2, 203, Hw, generator=g), wn_g=torch.randn(2, Hw, generator=g),
        seg=_segment(cfg, g, T, TP), pack=[_segment(cfg, g, t, tp) for t, tp in PACK])


def _to(m, x):
    if isinstance(x, dict):
        return {k: _to(m, v) for k, v in x.items()}
    if isinstance(x, list):
        return [_to(m, v) for v in x]
    return x.to(m.device, m.dtype)


def _ret(x):
    return x.detach().to("cpu", torch.float64)


def _cfg_context(m, s):
    """The (x, t)-independent half of one CFG-stacked velocity evaluation, as `cfm_inference` sets it up."""
    frames, tp = s["mu"].shape[1], s["prompt"].shape[-1]
    x = s["z"].clone()
    x[..., :tp] = 0
    prompt_x = torch.zeros_like(x)
    prompt_x[..., :tp] = s["prompt"]
    lens = torch.tensor([frames], device=m.device)
    ctx = m.dit_prepare(torch.cat([prompt_x, torch.zeros_like(prompt_x)], 0), lens, torch.cat([s["style"], torch.zeros_like(s["style"])], 0),
                        torch.cat([s["mu"], torch.zeros_like(s["mu"])], 0))
    return ctx, x, tp


def _tail(x, tp):
    return x[:, :, tp:]


@torch.no_grad()
def run(m, case, inp):
    """Output of one case on model m (fp64 CPU tensor).  `packed3_vs_segments` is `packed3` on every leg but the twin, where it is the
    per-segment `cfm_inference` of each segment: the device's packed solve against the twin's single-segment one."""
    i = _to(m, inp)
    if case.startswith("attention_T"):
        t = int(case[len("attention_T"):])
        return _ret(m._attention(i[f"qkv{t}"].clone(), 2, t, None))
    if case == "transformer":
        return _ret(m._transformer(i["tr_x"].clone(), i["tr_c"], None))
    if case == "wavenet":
        if m.device.type == "cuda":
            return _ret(m._wavenet_rows(i["wn_h"].clone(), i["wn_g"]) + m.wn_out_bias)
        ones = torch.ones(2, 1, 203, dtype=m.dtype)
        return _ret(m._wavenet(i["wn_h"].transpose(1, 2).clone(), ones, i["wn_g"], True).transpose(1, 2))
    if case in ("dit_step_window", "dit_step_full"):
        ctx, x, tp = _cfg_context(m, i["seg"])
        t = torch.full((2,), T_EVAL, device=m.device)
        return _ret(m.dit_step(ctx, x, t, out_from=tp if case == "dit_step_window" else 0))  # frames [Tp, T) / every frame
    segment = lambda s: _tail(m.cfm_inference(s["mu"], torch.tensor([s["mu"].shape[1]], device=m.device), s["prompt"], s["style"],  # noqa: E731
                                              STEPS, CFG_RATE, noise=s["z"]), s["prompt"].shape[-1])
    if case == "cfm3":
        return _ret(segment(i["seg"]))
    if case == "packed3" or (case == "packed3_vs_segments" and m.dtype != torch.float64):
        xs = m._cfm_packed(i["pack"], STEPS, CFG_RATE)
        return _ret(torch.cat([_tail(x, s["prompt"].shape[-1]) for x, s in zip(xs, i["pack"])], -1))
    if case == "packed3_vs_segments":
        return _ret(torch.cat([segment(s) for s in i["pack"]], -1))
    raise KeyError(case)


def rel_err(got, ref):
    """(max |got - ref| / max |ref|, rms(got - ref) / rms(ref)) against the twin's fp64 `ref`."""
    d = got.double() - ref
    return d.abs().max().item() / ref.abs().max().item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


class Legs:
    """The three legs of one configuration with the twin's outputs (`ref`) and the fp32 CPU leg's errors against them (`base`: case ->
    (max, rms)), computed once."""

    def __init__(self, name, device=None, cases=CASES):
        self.name = name
        self.cfg, self.cpu, self.twin, *rest = models(name, device)
        self.gpu = rest[0] if rest else None
        self.inp = inputs(self.cfg)
        self.ref, self.base = {}, {}
        for c in cases:
            self.ref[c] = run(self.twin, c, self.inp)
            # (on every leg but the twin the two packed cases are one computation)
            self.base[c] = rel_err(run(self.cpu, "packed3", self.inp), self.ref[c]) if c == "packed3_vs_segments" else \
                rel_err(run(self.cpu, c, self.inp), self.ref[c])

    def device(self, case, mode_name):
        """(max, rms) error of the device path against the twin in one arithmetic mode."""
        with mode(mode_name):
            return rel_err(run(self.gpu, case, self.inp), self.ref[case])
