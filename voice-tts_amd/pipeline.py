"""Host-side mirror of the hot loop of `IndexTTS2.infer_generator` (indextts/infer_v2.py:616-749)
for the two stages this repo builds: the autoregressive GPT (`inference_speech` + latent
`forward`) and the BigVGAN vocoder.  PyTorch is plumbing only (device tensors, the tiny
embedding gathers of `prepare_gpt_inputs`); all heavy arithmetic runs in libixtts_hip.so.

The stages between them that `north_star` leaves to PyTorch glue (conditioning encoders,
s2mel length-regulator + CFM) are NOT part of this package; callers hand in
`conds_latent` (model_v2.py:696) and the mel spectrogram (infer_v2.py:731).
"""
import numpy as np
import torch

from .bigvgan import BigVGAN
from .gpt_engine import GptEngine
from .weights import BIGVGAN_CFG, GPT_CFG

SAMPLE_RATE = 22050  # infer_v2.py:607


class _RawDeviceBuffer:
    """Expose a raw device pointer to torch without copying (for the RCCL weight broadcast)."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def arena_tensor(ptr, nbytes, device):
    return torch.as_tensor(_RawDeviceBuffer(ptr, nbytes), device=device)


def _text_rows(cfg, text_embedding, text_pos_embedding, text_ids, drop_inner=False):
    """[start] text [stop] embedded with its positions -> [L + 2, D] (model_v2.py:579-583,620-640); `drop_inner` first drops the
    start / stop text ids found inside the text, as `prepare_gpt_inputs` does."""
    t = torch.as_tensor(text_ids, dtype=torch.long, device=text_embedding.device).reshape(-1)
    start, stop = t.new_tensor([cfg["start_text_token"]]), t.new_tensor([cfg["stop_text_token"]])
    if drop_inner:
        t = t[(t != stop) & (t != start)]
    t = torch.cat((start, t, stop))
    return text_embedding[t] + text_pos_embedding[: t.numel()]


def prepare_gpt_inputs(cfg, text_embedding, text_pos_embedding, conds_latent, text_ids):
    """UnifiedVoice.prepare_gpt_inputs (model_v2.py:598-661), one sequence: start/stop text ids found INSIDE the text are
    dropped and made up for by zero rows on the left (mask 0 there), then [start] text [stop] is embedded.

    conds_latent [34, D] device; text_ids int [L].  Returns (embeds [P-1, D], n_left_pad, P)."""
    device = text_embedding.device
    temb = _text_rows(cfg, text_embedding, text_pos_embedding, text_ids, drop_inner=True)
    pad = torch.as_tensor(text_ids).numel() + 2 - temb.shape[0]
    parts = [conds_latent.to(device, torch.float32), temb]
    if pad > 0:
        parts.insert(0, torch.zeros(pad, temb.shape[1], device=device))
    embeds = torch.cat(parts, 0)
    return embeds, pad, embeds.shape[0] + 1


def conds_latent(cond32, emovec, speed_emb):
    """inference_speech (model_v2.py:693-696): the 32 conditioning rows plus the emotion vector, then the two speed rows -> [34, D].
    One implementation for `HotPath` and `IndexTTS2`."""
    dev = speed_emb.device
    c = cond32.to(dev, torch.float32) + emovec.to(dev, torch.float32).reshape(1, -1)
    return torch.cat((c, speed_emb[1:2], speed_emb[0:1]), 0)


def latent_prefix(cfg, text_embedding, text_pos_embedding, conds_latent, text_ids):
    """[conds ; text_emb] rows of UnifiedVoice.forward (model_v2.py:579-589); one implementation, as above."""
    return torch.cat((conds_latent.to(text_embedding.device, torch.float32), _text_rows(cfg, text_embedding, text_pos_embedding, text_ids)), 0)


def vocode(bigvgan, mel):
    """bigvgan(mel.float()) then the PCM clamp of infer_v2.py:735-744: fp32 [B, T] scaled to +-32767; one implementation, as above."""
    wav = bigvgan(mel.to(bigvgan.device_, torch.float32)).squeeze(1)
    return torch.clamp(32767 * wav, -32767.0, 32767.0)


def vocode_many(bigvgan, mels):
    """`vocode` for the mels of several segments ([1, 80, F_i], lengths unequal) -> one fp32 [1, T_i] per mel, in input order, or the
    EXCEPTION that mel raised.  A vocoder with `forward_many` (the built-in `BigVGAN`) takes them in batched passes; when such a pass
    raises, its mels are redone one at a time, so the exception lands only on the mel that caused it.  Any other vocoder (an
    injected stage, a test stub), or IXTTS_BV_BATCH=0: one `vocode` per mel."""
    from .bigvgan import plan_vocoder_batches, vocoder_batch_frames, vocoder_batching

    mels = list(mels)

    def one(mel):
        try:
            return vocode(bigvgan, mel)
        except Exception as e:  # this mel only
            return e

    if not hasattr(bigvgan, "forward_many") or not vocoder_batching() or len(mels) < 2:
        return [one(mel) for mel in mels]
    out = [None] * len(mels)
    # the groups `forward_many` would cut itself, cut here: one call and one failure domain per group
    for group in plan_vocoder_batches([mel.shape[-1] for mel in mels], vocoder_batch_frames()):
        try:
            wavs = bigvgan.forward_many([mels[i].to(bigvgan.device_, torch.float32) for i in group])
            for i, w in zip(group, wavs):
                out[i] = torch.clamp(32767 * w.squeeze(1), -32767.0, 32767.0)
        except Exception:
            for i in group:
                out[i] = one(mels[i])
    return out


def decode_segment(index, embeds, n_left_pad, max_new, request=0, payload=None, stream=None, sampler=None, bans=None, processors=None):
    """One prepared sequence as the decode schedulers take it (`scheduler.Segment`); `HotPath` and `IndexTTS2` build theirs here."""
    from .scheduler import Segment

    return Segment(request, index, embeds, n_left_pad, max_new, payload, stream, sampler, bans, processors)


class HotPath:
    def __init__(self, gpt_cfg=None, bigvgan_cfg=None, dtype="bf16", device="cuda:0", max_batch=2, max_seq=2048,
                 max_frames=2048, fast_sin=False):
        self.device = torch.device(device)
        self.gpt_cfg = dict(GPT_CFG if gpt_cfg is None else gpt_cfg)
        self.bigvgan_cfg = dict(BIGVGAN_CFG if bigvgan_cfg is None else bigvgan_cfg)
        self.gpt = GptEngine(self.gpt_cfg, dtype=dtype, max_seq=max_seq, max_batch=max_batch, device=self.device)
        self.bigvgan = BigVGAN(self.bigvgan_cfg, max_frames=max_frames, fast_sin=fast_sin, device=self.device)
        D = self.gpt_cfg["model_dim"]
        # glue tables for prepare_gpt_inputs / the latent prefix (model_v2.py:380,388-390,402)
        self.text_embedding = torch.zeros(self.gpt_cfg["number_text_tokens"] + 1, D, device=self.device)
        self.text_pos_embedding = torch.zeros(self.gpt_cfg["max_text_tokens"] + 2, D, device=self.device)
        self.speed_emb = torch.zeros(2, D, device=self.device)

    # ------------------------------------------------------------------ weights
    def load(self, gpt_sd, bigvgan_sd):
        self.gpt.load_state_dict(gpt_sd)
        self.bigvgan.load_state_dict(bigvgan_sd)
        self.text_embedding.copy_(gpt_sd["text_embedding.weight"])
        self.text_pos_embedding.copy_(gpt_sd["text_pos_embedding.emb.weight"])
        self.speed_emb.copy_(gpt_sd["speed_emb.weight"])
        return self

    def broadcast_tensors(self):
        """Device tensors that together hold every weight (rank 0 -> all, one call each)."""
        gp, gn = self.gpt.arena()
        bp, bn = self.bigvgan.arena()
        return [arena_tensor(gp, gn, self.device), arena_tensor(bp, bn, self.device), self.text_embedding,
                self.text_pos_embedding, self.speed_emb]

    def adopt(self):
        self.gpt.adopt_arena()
        self.bigvgan.adopt_arena()
        return self

    # ------------------------------------------------------------------ G0
    def prepare_gpt_inputs(self, conds_latent, text_ids):
        """-> (embeds [P-1, D], n_left_pad, P); see the module-level `prepare_gpt_inputs`."""
        return prepare_gpt_inputs(self.gpt_cfg, self.text_embedding, self.text_pos_embedding, conds_latent, text_ids)

    def conds_latent(self, cond32, emo_vec):
        """inference_speech (model_v2.py:693-696); see the module-level `conds_latent`."""
        return conds_latent(cond32, emo_vec, self.speed_emb)

    def latent_prefix(self, conds_latent, text_ids):
        """-> [34 + L + 2, D]; see the module-level `latent_prefix`."""
        return latent_prefix(self.gpt_cfg, self.text_embedding, self.text_pos_embedding, conds_latent, text_ids)

    # ------------------------------------------------------------------ G1-G8
    def generate(self, prompts, max_new, repetition_penalty=10.0, fixed_length=False, sync_every=64, **sampler):
        """Decode up to `max_batch` independent sequences together: greedy by default, multinomial sampling with
        `do_sample=True, temperature=, top_k=, top_p=, seed=` (each slot draws from its own counter-based stream).

        prompts: list of (embeds [P-1,D], n_left_pad).  Returns a list of int32 id arrays,
        trimmed at the first stop token (inclusive), as `generate()` would return them.
        """
        B = len(prompts)
        assert 1 <= B <= self.gpt.max_batch
        for b, (emb, pad) in enumerate(prompts):
            self.gpt.prefill(b, emb, pad)
        done = 0
        out = [None] * B
        while done < max_new:
            n = min(sync_every, max_new - done)
            self.gpt.decode(B, n, repetition_penalty=repetition_penalty, suppress_stop=fixed_length, **sampler)
            done += n
            fins = []
            for b in range(B):
                ids, fin = self.gpt.read(b)
                out[b] = ids[:max_new]
                fins.append(fin)
            if all(fins):
                break
        return out

    def generate_many(self, segments, fixed_length=False, repetition_penalty=10.0, sync_every=64):
        """Row N3: decode any number of segments (of any number of requests) with continuous batching over the engine's
        slots.  segments: list of (embeds [P-1,D], n_left_pad, max_new).  Returns the id arrays in submission order."""
        from .scheduler import DecodeScheduler

        out = [None] * len(segments)
        sched = DecodeScheduler(self.gpt, self.gpt.max_batch, self.gpt_cfg["stop_mel_token"], sync_every=sync_every)
        segs = [decode_segment(i, *s) for i, s in enumerate(segments)]
        self.last_sched_stats = sched.run(segs, lambda seg, ids: out.__setitem__(seg.index, ids), fixed_length=fixed_length,
                                          repetition_penalty=repetition_penalty)
        return out

    def generate_beams_many(self, segments, num_beams=3, fixed_length=False, sync_every=64, repetition_penalty=10.0, temperature=0.8,
                            top_k=30, top_p=0.8, seed=0, length_penalty=0.0, typical_mass=0.0):
        """The served default (`num_beams=3` beam-sample, infer_v2.py:598-606) for any number of segments: each segment is a
        beam group of `num_beams` slots, the engine's groups step together (a wide engine holds floor(max_batch / num_beams);
        up to 4 slots: one group, the segments in turn as the reference runs them).  segments: list of (embeds [P-1,D],
        n_left_pad, max_new).  Returns the best hypothesis per segment, in submission order."""
        from .scheduler import BeamGroupScheduler

        out = [None] * len(segments)
        sched = BeamGroupScheduler(self.gpt, num_beams, sync_every=sync_every)
        segs = [decode_segment(i, *s) for i, s in enumerate(segments)]
        self.last_sched_stats = sched.run(segs, lambda seg, ids, score: out.__setitem__(seg.index, ids), fixed_length=fixed_length,
                                          repetition_penalty=repetition_penalty, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                          length_penalty=length_penalty, typical_mass=typical_mass)
        return out

    # ------------------------------------------------------------------ G9
    def latent(self, conds_latent, text_ids, codes):
        prefix = self.latent_prefix(conds_latent, text_ids)
        codes = torch.as_tensor(np.asarray(codes), dtype=torch.int32, device=self.device)
        return self.gpt.latent(prefix, codes)

    def latent_many(self, items):
        """`latent` of several segments in packed passes (GptEngine.latent_many): items = [(conds_latent, text_ids, codes), ...]
        -> [latent [n_i, D], ...], each bit for bit what `latent` of the item returns."""
        entries = [(self.latent_prefix(cl, text_ids), torch.as_tensor(np.asarray(codes), dtype=torch.int32, device=self.device))
                   for cl, text_ids, codes in items]
        return self.gpt.latent_many(entries)

    # ------------------------------------------------------------------ N2 (PyTorch glue, optional)
    def attach_conditioning(self, W, cfg=None):
        """Conformer/perceiver conditioning encoders (voice-tts_amd/conditioning.py); W keyed like UnifiedVoice.state_dict()."""
        from .conditioning import COND_CFG, Conditioning

        self.cond_model = Conditioning(W, COND_CFG if cfg is None else cfg, device=self.device)
        return self

    @torch.no_grad()
    def conds_from_prompt(self, spk_cond_emb, emo_cond_emb=None, emo_alpha=1.0):
        """infer_v2.py:629-635 + model_v2.py:684-696: w2v-bert features [1,T,1024] of the speaker (and emotion) prompt ->
        conds_latent [34, D].  Once per request (the reference recomputes it per segment)."""
        cond32, emovec = self.cond_model.encode_prompt(spk_cond_emb, emo_cond_emb, emo_alpha)
        return self.conds_latent(cond32, emovec)

    # ------------------------------------------------------------------ N1 (PyTorch glue, optional)
    def attach_s2mel(self, W, cfg=None):
        """Semantic-to-mel stage (length regulator + CFM/DiT) as PyTorch-ROCm glue on this device (voice-tts_amd/s2mel.py)."""
        from .s2mel import S2MEL_CFG, S2Mel

        self.s2mel_model = S2Mel(W, S2MEL_CFG if cfg is None else cfg, device=self.device)
        return self

    def s2mel(self, latent, codes, prompt_condition, ref_mel, style, n_timesteps=25, inference_cfg_rate=0.7, noise=None, frames=None):
        """infer_v2.py:713-731: latent [n,D] + codes [n] -> mel [1,80,F] (fp32, as the reference runs this stage); F =
        `s2mel.target_frames(n)`, or `frames` (e.g. `target_frames(n, speed)`: the speaking rate)."""
        codes = torch.as_tensor(np.asarray(codes), dtype=torch.long, device=self.device).reshape(1, -1)
        lens = torch.tensor([codes.shape[1]], device=self.device)
        kw = {} if frames is None else dict(frames=frames)
        return self.s2mel_model(latent.reshape(1, codes.shape[1], -1), codes, lens, prompt_condition, ref_mel, style,
                                n_timesteps=n_timesteps, inference_cfg_rate=inference_cfg_rate, noise=noise, **kw)

    def s2mel_many(self, segments, n_timesteps=25, inference_cfg_rate=0.7, noises=None, frames=None):
        """`s2mel` for several segments in ONE packed CFM solve (S2Mel.solve_many): segments are (latent [n,D], codes [n],
        prompt_condition, ref_mel, style) tuples; returns one mel [1,80,F_i] per segment, F_i = `s2mel.target_frames(n_i)` or
        `frames[i]` where that is not None."""
        items = []
        for latent, codes, prompt_condition, ref_mel, style in segments:
            codes = torch.as_tensor(np.asarray(codes), dtype=torch.long, device=self.device).reshape(1, -1)
            items.append((latent.reshape(1, codes.shape[1], -1), codes, prompt_condition, ref_mel, style))
        kw = {} if frames is None else dict(frames=frames)
        return self.s2mel_model.solve_many(items, n_timesteps=n_timesteps, inference_cfg_rate=inference_cfg_rate, noises=noises, **kw)

    # ------------------------------------------------------------------ V0-V5
    def vocode(self, mel):
        """-> fp32 [1, T] scaled to +-32767; see the module-level `vocode`."""
        return vocode(self.bigvgan, mel)

    def vocode_many(self, mels):
        """One fp32 [1, T_i] (or the exception it raised) per mel; see the module-level `vocode_many`."""
        return vocode_many(self.bigvgan, mels)


def audio_seconds(n_codes_per_segment, interval_silence_ms=200, speed=1.0):
    """Audio length the reference produces for these code counts (infer_v2.py:719,752-754); `speed`: at that speaking rate."""
    from .s2mel import target_frames

    total = 0.0
    for n in n_codes_per_segment:
        frames = target_frames(n, None if speed == 1.0 else speed)
        total += frames * 256 / SAMPLE_RATE
    total += (len(n_codes_per_segment) - 1) * interval_silence_ms / 1000.0
    return total
