"""Recorded outputs of `IndexTTS2.infer`, `infer(stream_return=True)` and `infer_many` for tests/test_gpu_infer_parent.py: run ONCE, on
a GPU, at the commit whose results the request path has to keep (the parent of the change that gave `infer_generator` and
`infer_many` one implementation of every step), never regenerated from the code under test:

    python tests/golden/make_golden_infer_parent.py [path]     # -> tests/golden/infer_parent.npz

The recorder uses only what that parent has: the public entry points, the prompt-cache attributes and `m.gpt.latent`, which it wraps
to log the mel codes every segment hands to the latent pass.  Every case reseeds torch and the fake glue's generator and clears the
prompt caches first, so a case does not depend on the ones before it.

Per case the file holds each segment's codes (int32, in the order the latent pass saw them) and, per returned audio, the PCM length,
the sha256 of the int16 PCM bytes and the first 4096 samples; for the generator case the chunk lengths and the sha256 of the
concatenated chunks; for a request of `infer_many` that failed or had no text, the exception's type name or "None".

Models (`Models`): the fake-glue model of tests/test_gpu_infer_v2.py (tiny GPT 128 x 2 layers, BigVGAN 64, max_seq 192, max_frames
128) in fp32 and with `use_fp16=True` (bf16, wide engine), and the model-directory model of tests/synthetic_model_dir.py in fp32."""
import hashlib
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))  # tests/: synthetic_model_dir
PATH = os.path.join(HERE, "infer_parent.npz")
HEAD = 4096
TEXT72 = "abcdefghijklmnopqrstuvwxyz0123456789" * 2  # 72 ids -> 3 segments of <= 30
VEC = [0.1, 0, 0, 0, 0, 0, 0, 0.2]
DIR_TEXT = "Hello world, this is a test. 你好世界！"  # 2 segments of <= 20 tokens


class FakeGlue:
    """The deterministic glue of tests/test_gpu_infer_v2.py; the speaker prompt "bad.wav" cannot be encoded."""

    def __init__(self, D, dev):
        self.D, self.dev = D, dev
        self.g = torch.Generator().manual_seed(5)

    def tokenize(self, text, max_text_tokens_per_segment, quick_streaming_tokens=0):
        ids = [2 + (ord(c) % 190) for c in text]
        return [ids[i:i + max_text_tokens_per_segment] for i in range(0, len(ids), max_text_tokens_per_segment)]

    def speaker(self, spk_audio_prompt):
        if spk_audio_prompt == "bad.wav":
            raise ValueError("bad.wav: not audio")
        return dict(spk_cond_emb=torch.randn(1, 20, 16, generator=self.g).to(self.dev), style=torch.randn(1, 192, generator=self.g).to(self.dev),
                    prompt_condition=None, ref_mel=None)

    def emotion(self, emo_audio_prompt):
        return torch.randn(1, 20, 16, generator=self.g).to(self.dev)

    def emo_vector_mix(self, emo_vector, style, use_random):
        w = torch.tensor(emo_vector)
        return torch.full((1, self.D), 0.01 * float(w.sum()), device=self.dev), float(w.sum())

    def merge_emovec(self, spk_cond_emb, emo_cond_emb, alpha):
        base = spk_cond_emb.mean(dim=(1, 2)).reshape(1, 1).expand(1, self.D)
        emo = emo_cond_emb.mean(dim=(1, 2)).reshape(1, 1).expand(1, self.D)
        return (base + alpha * (emo - base)).contiguous()

    def get_conditioning(self, spk_cond_emb):
        return torch.linspace(-0.5, 0.5, 32 * self.D, device=self.dev).reshape(32, self.D)

    def s2mel(self, latent, codes, code_lens, speaker):
        F = int(int(code_lens[0]) * 1.72)
        assert latent.shape == (1, codes.shape[1], self.D)
        mel = (torch.randn(1, 80, F, generator=torch.Generator().manual_seed(F)) * 2 - 4).clamp(-11.5, 2)
        return mel.to(self.dev)


class Models:
    """The three models, each built when a case first asks for it."""

    def __init__(self, root=None):
        self._m, self._root = {}, root

    def __call__(self, name):
        if name not in self._m:
            self._m[name] = self._fake(name == "fake16") if name.startswith("fake") else self._from_dir()
        return self._m[name]

    @staticmethod
    def _fake(fp16):
        import voice_tts_amd.weights as WR
        from indextts.infer_v2 import IndexTTS2

        gcfg, bcfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2), WR.tiny_bigvgan_cfg(64)
        return IndexTTS2(cfg_path=None, model_dir="/nonexistent", use_fp16=fp16, device="cuda:0", use_cuda_kernel=True,
                         glue=FakeGlue(128, torch.device("cuda:0")), gpt_state_dict=WR.make_gpt_weights(gcfg, seed=7),
                         bigvgan_state_dict=WR.make_bigvgan_weights(bcfg, seed=8), gpt_cfg=gcfg, bigvgan_cfg=bcfg, max_seq=192, max_frames=128)

    def _from_dir(self):
        import synthetic_model_dir as SM
        from indextts.infer_v2 import IndexTTS2
        from voice_tts_amd.front import TextNormalizer, TextTokenizer

        root = self._root or tempfile.mkdtemp(prefix="infer_parent_model_dir")
        cfg_path, _ = SM.write_model_dir(root)

        class Same:
            def normalize(self, s):
                return s

        tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
        return IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=False, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256)


def _dir_wavs():
    import synthetic_model_dir as SM

    return SM.synthetic_wav_bytes(1.5, 24000), SM.synthetic_wav_bytes(1.0, 16000, seed=1), SM.synthetic_wav_bytes(1.2, 16000, seed=2)


def cases():
    """[(id, model, kind, call)]: kind is "infer", "stream" or "many"; `call(m)` makes the request."""
    greedy = dict(num_beams=1, top_k=1)

    def m1(m):
        a, _, e = _dir_wavs()
        return m.infer(a, DIR_TEXT, None, emo_audio_prompt=e, emo_alpha=0.7, max_text_tokens_per_segment=20, max_mel_tokens=20, **greedy)

    def m3(m):
        return m.infer(_dir_wavs()[0], DIR_TEXT, None, max_text_tokens_per_segment=20, max_mel_tokens=20, **greedy)

    def m4(m):
        a, b, _ = _dir_wavs()
        return m.infer_many([dict(spk_audio_prompt=a, text=DIR_TEXT), dict(spk_audio_prompt=b, text="Short.")], max_text_tokens_per_segment=20,
                            decode_slots=4, max_mel_tokens=20, **greedy)

    return [
        ("F1", "fake", "infer", lambda m: m.infer("spk.wav", TEXT72, None, max_text_tokens_per_segment=30, max_mel_tokens=20, **greedy)),
        ("F2", "fake", "infer", lambda m: m.infer("spk.wav", "hello world", None, max_mel_tokens=12, **greedy)),
        ("F3", "fake", "infer", lambda m: m.infer("spk.wav", "abcdefghij" * 2, None, emo_vector=VEC, emo_alpha=0.5, seed=11, max_mel_tokens=16)),
        ("F4", "fake", "stream", lambda m: m.infer("spk2.wav", "abcdefghij" * 5, None, max_text_tokens_per_segment=25, stream_return=True,
                                                   max_mel_tokens=16, seed=11)),
        ("F5", "fake", "infer", lambda m: m.infer("spk.wav", "abcdefghij" * 5, None, emo_audio_prompt="emo.wav", emo_alpha=0.7,
                                                  max_text_tokens_per_segment=25, num_beams=1, top_k=30, seed=5, max_mel_tokens=16)),
        ("F6", "fake", "many", lambda m: m.infer_many(
            [dict(spk_audio_prompt="a.wav", text=TEXT72), dict(spk_audio_prompt="b.wav", text="hello world", emo_vector=VEC, emo_alpha=0.5),
             dict(spk_audio_prompt="a.wav", text="")], max_text_tokens_per_segment=30, decode_slots=4, max_mel_tokens=16, **greedy)),
        ("F7", "fake", "many", lambda m: m.infer_many(
            [dict(spk_audio_prompt="a.wav", text="abcdefghij" * 5), dict(spk_audio_prompt="b.wav", text="hello world", emo_audio_prompt="emo.wav",
                                                                         emo_alpha=0.7)],
            max_text_tokens_per_segment=25, decode_slots=3, seed=2, max_mel_tokens=16)),
        ("F8", "fake16", "infer", lambda m: m.infer("spk.wav", TEXT72, None, max_text_tokens_per_segment=30, seed=4, max_mel_tokens=24)),
        ("F9", "fake16", "many", lambda m: m.infer_many(
            [dict(spk_audio_prompt="a.wav", text="abcdefghij" * 5), dict(spk_audio_prompt="bad.wav", text="broken prompt"),
             dict(spk_audio_prompt="b.wav", text="hello world")], max_text_tokens_per_segment=25, decode_slots=9, seed=2, max_mel_tokens=16)),
        ("M1", "dir", "infer", m1),
        ("M2", "dir", "infer", m1),  # under IXTTS_S2MEL_BATCH=1
        ("M3", "dir", "infer", m3),
        ("M4", "dir", "many", m4),
    ]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _audio(rec, key, res):
    if not isinstance(res, tuple):
        rec[key + "/result"] = np.array("None" if res is None else type(res).__name__)
        return
    sr, pcm = res
    assert sr == 22050 and pcm.dtype == np.int16 and pcm.ndim == 2 and pcm.shape[1] == 1
    rec[key + "/len"] = np.array(pcm.shape[0], dtype=np.int64)
    rec[key + "/sha256"] = np.array(_sha(pcm.astype("<i2")))
    rec[key + "/head"] = pcm[:HEAD, 0].copy()


def run_case(cid, kind, call, m):
    """One case on model `m` -> {key: array} as the file stores it (keys start with the case id)."""
    torch.manual_seed(1234)
    if m.glue is not None:
        m.glue.g.manual_seed(5)
    m.cache_spk_audio_prompt = m.cache_spk = m.cache_emo_audio_prompt = m.cache_emo_cond = None
    seen, real = [], m.gpt.latent

    def latent(prefix, codes):
        seen.append(torch.as_tensor(codes).detach().cpu().numpy().astype(np.int32).reshape(-1))
        return real(prefix, codes)

    batch = os.environ.pop("IXTTS_S2MEL_BATCH", None)
    if cid == "M2":
        os.environ["IXTTS_S2MEL_BATCH"] = "1"
    m.gpt.latent = latent
    try:
        res = call(m)
        if kind == "stream":
            res = list(res)
    finally:
        del m.gpt.latent  # the instance attribute that shadowed the method
        os.environ.pop("IXTTS_S2MEL_BATCH", None)
        if batch is not None:
            os.environ["IXTTS_S2MEL_BATCH"] = batch
    rec = {f"{cid}/n_segments": np.array(len(seen), dtype=np.int64)}
    for i, c in enumerate(seen):
        rec[f"{cid}/codes/{i}"] = c
    if kind == "infer":
        _audio(rec, cid, res)
    elif kind == "many":
        rec[f"{cid}/n_requests"] = np.array(len(res), dtype=np.int64)
        for j, r in enumerate(res):
            _audio(rec, f"{cid}/r{j}", r)
    else:
        assert all(isinstance(c, torch.Tensor) and c.dtype == torch.float32 and c.device.type == "cpu" for c in res)
        rec[f"{cid}/chunk_lens"] = np.array([c.shape[1] for c in res], dtype=np.int64)
        rec[f"{cid}/sha256"] = np.array(_sha(torch.cat(res, dim=1).type(torch.int16).numpy().astype("<i2")))
        rec[f"{cid}/sha256_f32"] = np.array(_sha(torch.cat(res, dim=1).numpy()))
    return rec


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    models, rec = Models(), {}
    for cid, model, kind, call in cases():
        out = run_case(cid, kind, call, models(model))
        rec.update(out)
        print(cid, {k: (v.tolist() if v.ndim == 0 or v.size <= 8 else v.shape) for k, v in out.items() if "/codes/" not in k and not k.endswith("/head")},
              flush=True)
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
