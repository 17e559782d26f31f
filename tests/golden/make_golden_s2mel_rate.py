"""tests/golden/s2mel_rate.npz: the REFERENCE's length regulator and CFM at other frame counts than floor(1.72 n) -- the speaking rate.

    python tests/golden/make_golden_s2mel_rate.py

The `s2mel_hd64` twin of make_golden.py (hidden 128, 2 heads: head_dim 64, so the HIP attention runs), n = 90 codes, Tp = 70 prompt
frames.  Per speed in SPEEDS the reference's `length_regulator` is called with `ylens = (code_lens * 1.72 / speed).long()` and its
`cfm.inference` with 2 steps; `inference` draws its noise itself, so its one `torch.randn` call is handed the draw that is stored as
`noise`.  Stored per speed: `cond_<k>`, `noise_<k>` (the frames behind the prompt: the solve zeroes the prompt's), `mel_<k>`;
the shared inputs once.  The latent and the noise are rounded to fp16 values before use and stored as fp16 (the file stays small).

A regulator-only sweep: `cond` of the first n codes for short (n, speed) whose frame counts F put Tp' + F = 63, 64, 65 rows (Tp' = 30)
on both sides of a 64-row tile of the packed attention (`sweep_n`, `sweep_speed`, `sweep_frames`, `sweep_cond_<j>`).

Data only: no reference text is written anywhere."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import build_ref_s2mel, save  # noqa: E402  (installs the reference import harness)

SPEEDS = (0.5, 0.8, 1.25, 2.0)
SWEEP = ((24, 1.25), (10, 0.5), (25, 1.25), (41, 2.0), (38, 2.0))  # F = 33, 34, 34, 35, 32
SWEEP_TP = 30
N_STEPS = 2


def main(name="s2mel_rate.npz", seed=173, n=90, Tp=70):
    import voice_tts_amd.s2mel as S2

    cfg = S2.tiny_s2mel_cfg(gpt_dim=1280, semantic_dim=1024, lr_in_channels=1024, codebook_size=8194, hidden_dim=128, num_heads=2,
                            wavenet_hidden=128, depth=3)
    W = S2.make_s2mel_weights(cfg, seed=seed)
    code_lens = torch.tensor([n])
    frames = [int((code_lens * 1.72 / sp).long()) for sp in SPEEDS]
    m, q = build_ref_s2mel(cfg, W, Tp + max(frames))
    g = torch.Generator().manual_seed(seed + 1)
    latent = (torch.randn(1, n, 1280, generator=g) * 0.5).half().float()
    codes = torch.randint(0, 8192, (1, n), generator=g)
    prompt_condition = torch.randn(1, Tp, cfg["content_dim"], generator=g)
    ref_mel = torch.randn(1, 80, Tp, generator=g) * 2 - 4
    style = torch.randn(1, cfg["style_dim"], generator=g)
    S_infer = q.vq2emb(codes).transpose(1, 2) + m.models["gpt_layer"](latent)
    out = dict(seed=seed, n_steps=N_STEPS, speeds=np.array(SPEEDS), frames=np.array(frames), latent=latent.half(), codes=codes,
               prompt_condition=prompt_condition, ref_mel=ref_mel, style=style)
    cfm = m.models["cfm"]
    for k, (sp, F) in enumerate(zip(SPEEDS, frames)):
        ylens = (code_lens * 1.72 / sp).long()
        cond = m.models["length_regulator"](S_infer, ylens=ylens, n_quantizers=3, f0=None)[0]
        assert cond.shape[1] == F
        cat = torch.cat([prompt_condition, cond], dim=1)
        T = cat.shape[1]
        # `inference` draws its noise itself: the draw is made here (fp16 values, so that the stored half reproduces it) and handed
        # to it in place of its one `torch.randn` call
        torch.manual_seed(seed + 10 + k)
        noise = torch.randn(1, 80, T).half().float()
        real = torch.randn
        torch.randn = lambda *a, **kw: noise.clone()  # (the one draw of `inference`: [B, in_channels, T])
        try:
            mel = cfm.inference(cat, torch.LongTensor([T]), ref_mel, style, None, N_STEPS, inference_cfg_rate=0.7)
        finally:
            torch.randn = real
        out[f"cond_{k}"], out[f"noise_{k}"], out[f"mel_{k}"] = cond, noise[:, :, Tp:].half(), mel[:, :, Tp:]
        print(f"speed {sp}: {F} frames, mel range {float(mel[:, :, Tp:].min()):.3f} .. {float(mel[:, :, Tp:].max()):.3f}")
    sweep_frames = []
    for j, (ns, sp) in enumerate(SWEEP):
        ylens = (torch.tensor([ns]) * 1.72 / sp).long()
        cond = m.models["length_regulator"](S_infer[:, :ns], ylens=ylens, n_quantizers=3, f0=None)[0]
        sweep_frames.append(int(ylens))
        out[f"sweep_cond_{j}"] = cond
    assert {SWEEP_TP + f for f in sweep_frames} >= {63, 64, 65}, sweep_frames
    out.update(sweep_n=np.array([s[0] for s in SWEEP]), sweep_speed=np.array([s[1] for s in SWEEP]), sweep_frames=np.array(sweep_frames),
               sweep_tp=SWEEP_TP)
    save(name, **out)


if __name__ == "__main__":
    main()
