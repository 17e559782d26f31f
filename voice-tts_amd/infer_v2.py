"""Host-side mirror of `indextts.infer_v2.IndexTTS2` for the hot path this repo builds.

Same constructor and `infer(...)` signature, return values, wav format and log lines as the
reference (`indextts/infer_v2.py:36-45,438-461,463-783`).  The two hot stages -- the GPT
(`inference_speech` + latent `forward`) and BigVGAN -- run in libixtts_hip.so; the stages
`north_star` leaves to PyTorch glue run on the same device through this package's torch
restatements: conformer/perceiver conditioners (`conditioning.py`), s2mel length regulator + CFM
(`s2mel.py`), and the once-per-prompt stages of infer_v2.py:508-580 (`prompt.py`: audio decode of
the five prompt forms, resampling, w2v-bert features through the installed `transformers`
classes, semantic codec `quantize`, reference mel, kaldi fbank + CAM++, emotion-matrix mix).

`IndexTTS2(cfg_path, model_dir).infer(wav, text)` therefore runs from the files of `model_dir`
alone (layout in INTEGRATION.md; nothing is ever downloaded); every component can also be handed
in as tensors (`*_state_dict=`, `w2v_bert=`, `emo_matrix=` ...), which is how the tests and the
bench build synthetic twins.  A `glue=` object still overrides any stage (see `Glue`).  There is
no silent fallback: a stage whose weights are missing makes `infer()` raise, naming the file.
"""
import logging
import os
import time
import warnings
import wave
from types import SimpleNamespace

import numpy as np
import torch

from .bigvgan import BigVGAN
from .gpt_engine import GptEngine, generation_constraints, generation_processors, resolve_gpt_dtype, resolve_min_length
from . import output as _output  # (through the module: a test may wrap `finish`)
from .pipeline import conds_latent, decode_segment, latent_prefix, prepare_gpt_inputs, vocode, vocode_many
from .s2mel import check_speed, target_frames
from .weights import BIGVGAN_CFG, GPT_CFG, load_bigvgan_checkpoint, load_gpt_checkpoint

logger = logging.getLogger("indextts.infer_v2")


def s2mel_batching():
    """IXTTS_S2MEL_BATCH=1: the CFM solves of several segments as ONE packed solve (S2Mel.solve_many).  Off by default: at the
    headline's 2 x 1100 codes the packed solve is 2.6 % slower than two per-segment solves (profiles/r05_notes.md)."""
    return os.environ.get("IXTTS_S2MEL_BATCH", "0") == "1"


def _same_prompt(a, b):
    """The reference's cache test `cache_spk_audio_prompt != spk_audio_prompt` (infer_v2.py:508,566) for every prompt form:
    equal paths / bytes hit the cache even when they are distinct objects; arrays and tensors compare by content."""
    if a is b:
        return True
    if type(a) is not type(b):
        return False
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same_prompt(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and bool(np.array_equal(a, b))
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and bool(torch.equal(a, b))
    try:
        return bool(a == b)
    except Exception:
        return False


def load_s2mel_checkpoint(path):
    """`load_checkpoint2` (s2mel/modules/commons.py:568-624): {"net": {module: state_dict}}, DDP "module." prefixes stripped;
    flattened to `module.key` as `S2Mel` reads them.  Tensors only (weights_only)."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    net = sd["net"] if "net" in sd else sd
    out = {}
    for mod, params in net.items():
        if not isinstance(params, dict):
            continue
        for k, v in params.items():
            k = k[7:] if k.startswith("module.") else k
            if torch.is_tensor(v) and v.is_floating_point():
                out[f"{mod}.{k}"] = v.float()
    return out


def _s2mel_cfg_from_yaml(y, base):
    """`cfg.s2mel` (Appendix A layout) -> the keys `S2Mel` reads."""
    c = dict(base)
    d, w, lr = y.get("DiT") or {}, y.get("wavenet") or {}, y.get("length_regulator") or {}
    for src, dst in (("hidden_dim", "hidden_dim"), ("num_heads", "num_heads"), ("depth", "depth"), ("in_channels", "in_channels"), ("content_dim", "content_dim")):
        if src in d:
            c[dst] = d[src]
    for src, dst in (("hidden_dim", "wavenet_hidden"), ("num_layers", "wavenet_layers"), ("kernel_size", "wavenet_kernel"), ("dilation_rate", "wavenet_dilation_rate")):
        if src in w:
            c[dst] = w[src]
    if "channels" in lr:
        c["lr_channels"] = lr["channels"]
    if "in_channels" in lr:
        c["lr_in_channels"] = lr["in_channels"]
    if "sampling_ratios" in lr:
        c["lr_n_blocks"] = len(lr["sampling_ratios"])
    if "dim" in (y.get("style_encoder") or {}):
        c["style_dim"] = y["style_encoder"]["dim"]
    return c


class Glue:
    """Optional override of the PyTorch-hosted stages: a method that is implemented
    replaces the built-in stage, one that raises NotImplementedError leaves the built-in in place.  All tensors on `device`."""

    def tokenize(self, text, max_text_tokens_per_segment, quick_streaming_tokens=0):
        """-> list of segments, each a list of text token ids (front.py:313-327,345-436; infer_v2.py:582-583,617)."""
        raise NotImplementedError

    def speaker(self, spk_audio_prompt):
        """-> dict(spk_cond_emb [1,T,1024], style [1,192], prompt_condition [1,Tr,512], ref_mel [1,80,Tr]) (infer_v2.py:508-545)."""
        raise NotImplementedError

    def emotion(self, emo_audio_prompt):
        """-> emo_cond_emb [1,T,1024] (infer_v2.py:565-580)."""
        raise NotImplementedError

    def emo_vector_mix(self, emo_vector, style, use_random):
        """-> (emovec_mat [1,D], weight_sum) (infer_v2.py:552-563)."""
        raise NotImplementedError

    def merge_emovec(self, spk_cond_emb, emo_cond_emb, alpha):
        """UnifiedVoice.merge_emovec -> [1,D] (model_v2.py:742-747).  Only called when the GPT checkpoint lacks the encoders."""
        raise NotImplementedError

    def get_conditioning(self, spk_cond_emb):
        """UnifiedVoice.get_conditioning -> [32,D] (model_v2.py:514-543,684).  Only called when the GPT checkpoint lacks the encoders."""
        raise NotImplementedError

    def s2mel(self, latent, codes, code_lens, speaker):
        """gpt_layer + vq2emb + length_regulator + cfm.inference -> mel [1,80,F] after the prompt (infer_v2.py:713-731).
        Only called when no `s2mel_state_dict` was given."""
        raise NotImplementedError


class IndexTTS2:
    returns_pcm_without_path = True  # infer(output_path=None) -> (22050, int16 [N, 1]) (infer_v2.py:776-783): the server skips the temp file

    def __init__(self, cfg_path="models/IndexTTS/config.yaml", model_dir="models/IndexTTS", use_fp16=False, device=None,
                 use_cuda_kernel=None, use_deepspeed=False, *, glue=None, gpt_state_dict=None, bigvgan_state_dict=None,
                 s2mel_state_dict=None, gpt_cfg=None, bigvgan_cfg=None, cond_cfg=None, s2mel_cfg=None, tokenizer=None,
                 max_seq=2048, max_frames=4096, w2v_bert=None, w2v_stats=None, semantic_codec_state_dict=None, codec_cfg=None,
                 campplus_state_dict=None, emo_matrix=None, spk_matrix=None, emo_num=None, weight_broadcast=None, qwen_emo=None,
                 qwen_emo_dtype="f16", gpt_dtype=None):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("the HIP hot path needs a GPU (no CPU fallback); pass device='cuda:N'")
            device = "cuda:0"
        self.device = torch.device(device)
        self.use_fp16 = bool(use_fp16)
        self.use_cuda_kernel = True if use_cuda_kernel is None else bool(use_cuda_kernel)
        if use_deepspeed:
            logger.info("use_deepspeed is ignored: the HIP decode engine stands in DeepSpeed's seam (model_v2.py:433-446)")
        self.model_dir = model_dir
        self.glue = glue
        gcfg, bcfg = dict(GPT_CFG if gpt_cfg is None else gpt_cfg), dict(BIGVGAN_CFG if bigvgan_cfg is None else bigvgan_cfg)
        cfg = {}
        if cfg_path and os.path.isfile(cfg_path):
            import yaml

            cfg = yaml.safe_load(open(cfg_path)) or {}
            for k in gcfg:
                if k in cfg.get("gpt", {}):
                    gcfg[k] = cfg["gpt"][k]
        self.cfg = cfg
        self.model_version = cfg.get("version")
        self.stop_mel_token = gcfg["stop_mel_token"]
        # reference precision: fp16 GPT under use_fp16 (infer_v2.py:79,88-89); here bf16 is the throughput mode and the default,
        # gpt_dtype="f16" / IXTTS_GPT_DTYPE=f16 gives the reference's IEEE half (resolve_gpt_dtype)
        self.gpt_dtype = resolve_gpt_dtype(self.use_fp16, gpt_dtype)
        from .scheduler import resolve_batch_prefill, resolve_latent_batch

        self.prefill_batch = resolve_batch_prefill()  # IXTTS_PREFILL_BATCH: refill rounds of the decode schedulers as one packed prefill
        self.latent_batch = resolve_latent_batch()  # IXTTS_LATENT_BATCH: the latents of a call's segments in packed passes (latent_many)
        self.gpt = GptEngine(gcfg, dtype=self.gpt_dtype, max_seq=max_seq, max_batch=3, device=self.device)
        # ---- weights: rank 0 (or a lone worker) reads model_dir; with `weight_broadcast=(rank, world)` (torch.distributed initialised,
        # backend nccl = RCCL over xGMI) the other workers of the node read nothing but config.yaml / bpe.model / the w2v-bert
        # directory: the glue tensors arrive as one packed message, the GPT and BigVGAN weights as their packed device arenas
        # (north_star: "RCCL over xGMI only for weight broadcast at load"; the reference's workers each read the files, server.py:28-77)
        self._bc = weight_broadcast
        peer = weight_broadcast is not None and int(weight_broadcast[0]) != 0
        files = dict(gpt=gpt_state_dict, bigvgan=bigvgan_state_dict, s2mel=s2mel_state_dict, codec=semantic_codec_state_dict, campplus=campplus_state_dict,
                     emo_matrix=emo_matrix, spk_matrix=spk_matrix)
        if not peer:
            files, bcfg = self._read_model_dir(files, cfg, model_dir, bcfg, bigvgan_cfg is None)
        if weight_broadcast is not None:
            files, bcfg = self._exchange_glue(files, bcfg, peer)
        gpt_state_dict, bigvgan_state_dict, s2mel_state_dict = files["gpt"], files["bigvgan"], files["s2mel"]
        semantic_codec_state_dict, campplus_state_dict, emo_matrix, spk_matrix = files["codec"], files["campplus"], files["emo_matrix"], files["spk_matrix"]
        if gpt_state_dict is None:
            raise FileNotFoundError("no GPT weights: pass gpt_state_dict=... or provide model_dir/gpt_checkpoint (checkpoint.py:25-34)")
        if bigvgan_state_dict is None:
            raise FileNotFoundError("no BigVGAN weights: pass bigvgan_state_dict=... or provide model_dir/bigvgan_generator.pt")
        if bigvgan_cfg is None and "conv_pre.weight" in bigvgan_state_dict:
            bcfg["upsample_initial_channel"] = int(bigvgan_state_dict["conv_pre.weight"].shape[0])  # the one width the tensors fix
        self.bigvgan = BigVGAN(bcfg, use_cuda_kernel=True, max_frames=max_frames, device=self.device)
        if not peer:
            self.gpt.load_state_dict(gpt_state_dict)
            self.bigvgan.load_state_dict(bigvgan_state_dict)
        if weight_broadcast is not None:  # the packed device arenas: one RCCL broadcast each, then `adopt_arena` on the receivers
            from . import sharding
            from .pipeline import arena_tensor

            gp, gn = self.gpt.arena()
            bp, bn = self.bigvgan.arena()
            sharding.broadcast_weights([arena_tensor(gp, gn, self.device), arena_tensor(bp, bn, self.device)], src=0)
            torch.cuda.synchronize(self.device)
            if peer:
                self.gpt.adopt_arena()
                self.bigvgan.adopt_arena()
        self._engines = {}  # further engine shapes over the same device weights, by slot count (infer_many, beam groups)
        D = gcfg["model_dim"]
        self.text_embedding = gpt_state_dict["text_embedding.weight"].to(self.device, torch.float32)
        self.text_pos_embedding = gpt_state_dict["text_pos_embedding.emb.weight"].to(self.device, torch.float32)
        self.speed_emb = gpt_state_dict["speed_emb.weight"].to(self.device, torch.float32)
        self.gpt_cfg = gcfg
        self.model_dim = D
        # rows N2 / N1 as PyTorch-ROCm glue, when their weights are there
        self.cond = None
        if "conditioning_encoder.embed.conv.0.weight" in gpt_state_dict:
            from .conditioning import COND_CFG, Conditioning

            if cond_cfg is None:
                cond_cfg = dict(COND_CFG, model_dim=D)
                for k in ("condition_module", "emo_condition_module"):
                    if k in cfg.get("gpt", {}):
                        cond_cfg[k] = {**cond_cfg[k], **{a: b for a, b in cfg["gpt"][k].items() if a in cond_cfg[k]}}
                # widths the yaml does not spell out are read off the tensors
                # Conv2dSubsampling2.out is Linear(D * ((idim - 1) // 2), D) (subsampling.py:152-153): only (idim - 1) // 2 enters the
                # arithmetic; the even idim with that quotient is the feature size of w2v-bert (1024 -> 511)
                eo = gpt_state_dict["conditioning_encoder.embed.out.0.weight"]
                cond_cfg["input_size"] = cfg.get("gpt", {}).get("input_size", 2 * (eo.shape[1] // eo.shape[0]) + 2)
                cond_cfg["perceiver_dim_head"] = gpt_state_dict["perceiver_encoder.layers.0.0.to_q.weight"].shape[0] // cond_cfg["condition_module"]["attention_heads"]
                cond_cfg["perceiver_depth"] = len({k.split(".")[2] for k in gpt_state_dict if k.startswith("perceiver_encoder.layers.")})
                cond_cfg["cnn_kernel"] = gpt_state_dict["conditioning_encoder.encoders.0.conv_module.depthwise_conv.weight"].shape[-1]
                cond_cfg["emo_dim"] = gpt_state_dict["emovec_layer.weight"].shape[1]
                cond_cfg["cond_num"] = gpt_state_dict["perceiver_encoder.latents"].shape[0]
            self.cond = Conditioning(gpt_state_dict, cond_cfg, device=self.device)
        # ---- prompt-side models (prompt.py; infer_v2.py:114-152,168-188): given tensors, else the files of model_dir
        from . import prompt as PR

        missing = []
        have = lambda *parts: os.path.exists(os.path.join(model_dir, *parts))
        codec_cfg = dict(PR.CODEC_CFG if codec_cfg is None else codec_cfg)
        for k in codec_cfg:
            if k in (cfg.get("semantic_codec") or {}):
                codec_cfg[k] = cfg["semantic_codec"][k]
        self.semantic_codec = PR.SemanticCodec(semantic_codec_state_dict, codec_cfg, self.device) if semantic_codec_state_dict is not None else None
        if self.semantic_codec is None:
            missing.append("semantic_codec/model.safetensors")
        self.s2mel = None
        if s2mel_state_dict is not None:
            from .s2mel import S2MEL_CFG, S2Mel

            scfg = dict(S2MEL_CFG if s2mel_cfg is None else s2mel_cfg)
            if s2mel_cfg is None and cfg.get("s2mel"):
                scfg = _s2mel_cfg_from_yaml(cfg["s2mel"], scfg)
            s2mel_state_dict = dict(s2mel_state_dict)
            if "quantizer.codebook.weight" not in s2mel_state_dict and self.semantic_codec is not None:
                # `semantic_codec.quantizer.vq2emb` (infer_v2.py:714) lives in the codec checkpoint, not in s2mel.pth
                s2mel_state_dict.update(self.semantic_codec.s2mel_quantizer_tensors())
                scfg.update(codebook_size=codec_cfg["codebook_size"], codebook_dim=codec_cfg["codebook_dim"], semantic_dim=codec_cfg["hidden_size"])
            self.s2mel = S2Mel(s2mel_state_dict, scfg, device=self.device)
        else:
            missing.append(cfg.get("s2mel_checkpoint", "s2mel.pth"))
        if w2v_bert is not None and not isinstance(w2v_bert, PR.W2vBert):
            st = w2v_stats if w2v_stats is not None else {"mean": torch.zeros(1), "var": torch.ones(1)}
            w2v_bert = PR.W2vBert(w2v_bert, st["mean"], torch.sqrt(st["var"]), device=self.device)
        if w2v_bert is None and have("w2v-bert-2.0") and cfg.get("w2v_stat") and have(cfg["w2v_stat"]):
            w2v_bert = PR.W2vBert.from_dir(os.path.join(model_dir, "w2v-bert-2.0"), os.path.join(model_dir, cfg["w2v_stat"]), self.device)
        self.w2v_bert = w2v_bert
        if w2v_bert is None:
            missing.append("w2v-bert-2.0/ + " + str(cfg.get("w2v_stat", "wav2vec2bert_stats.pt")))
        self.campplus = PR.CamPlus(campplus_state_dict, self.device) if campplus_state_dict is not None else None
        if self.campplus is None:
            missing.append("campplus_cn_common.bin")
        self.prompt = None
        if not missing:
            sp = ((cfg.get("s2mel") or {}).get("preprocess_params") or {})
            spect = sp.get("spect_params") or {}
            mel_args = dict(n_fft=spect.get("n_fft", 1024), win_size=spect.get("win_length", 1024), hop_size=spect.get("hop_length", 256),
                            num_mels=spect.get("n_mels", 80), sampling_rate=sp.get("sr", 22050), fmin=spect.get("fmin", 0),
                            fmax=None if spect.get("fmax", "None") == "None" else 8000)
            self.prompt = PR.PromptEncoder(self.w2v_bert, self.semantic_codec, self.campplus, self.s2mel, self.device, mel_args)
        self.missing_glue = missing
        # emotion matrices (infer_v2.py:168-176): rows grouped per emotion by emo_num
        self.emo_num = list(emo_num if emo_num is not None else cfg.get("emo_num", []))
        for name, given, key in (("emo_matrix", emo_matrix, "emo_matrix"), ("spk_matrix", spk_matrix, "spk_matrix")):
            m = given
            setattr(self, name, torch.split(m.to(self.device), self.emo_num) if m is not None and self.emo_num else None)
        # text front-end (row N4; infer_v2.py:161-165): a given tokenizer, else model_dir/<dataset.bpe_model> with the
        # reference's normaliser (needs WeText, as there), else `glue.tokenize`
        self.tokenizer = tokenizer
        bpe = os.path.join(model_dir, (cfg.get("dataset") or {}).get("bpe_model", "")) if cfg.get("dataset") else None
        if self.tokenizer is None and bpe and os.path.isfile(bpe):
            from .front import TextNormalizer, TextTokenizer

            self.normalizer = TextNormalizer()
            try:
                self.normalizer.load()  # infer_v2.py:162-163: the WeText verbalisers, imported as the reference imports them
                self.tokenizer = TextTokenizer(bpe, self.normalizer)
                logger.info(f"bpe model loaded from: {bpe}")
            except ImportError as e:
                self.missing_glue.append(f"text normalizer (WeTextProcessing not importable: {e})")
        # text emotion model (infer_v2.py:82): a given QwenEmotion or directory, else model_dir/<qwen_emo_path> when it exists.
        # Every worker reads it itself (also under weight_broadcast).  fp16 weights as the reference loads them.
        self.qwen_emo_dir = os.path.join(model_dir, cfg["qwen_emo_path"]) if cfg.get("qwen_emo_path") else None
        if qwen_emo is None and self.qwen_emo_dir and os.path.isdir(self.qwen_emo_dir):
            qwen_emo = self.qwen_emo_dir
        if qwen_emo is not None and not hasattr(qwen_emo, "inference"):
            from .qwen_emotion import QwenEmotion

            qwen_emo = QwenEmotion(qwen_emo, dtype=qwen_emo_dtype, device=self.device)
        self.qwen_emo = qwen_emo
        # prompt caches (infer_v2.py:190-197)
        self.cache_spk_audio_prompt = None
        self.cache_spk = None
        self.cache_emo_audio_prompt = None
        self.cache_emo_cond = None

    # ------------------------------------------------------------------ weights: files on rank 0, RCCL everywhere else
    @staticmethod
    def _read_model_dir(files, cfg, model_dir, bcfg, derive_bcfg):
        """Whatever was not handed in as a tensor dict is read from model_dir (INTEGRATION.md layout); tensors only
        (`weights_only=True` / safetensors).  Returns (files, bigvgan cfg)."""
        have = lambda *parts: os.path.exists(os.path.join(model_dir, *parts))
        if files["gpt"] is None and cfg.get("gpt_checkpoint") and os.path.isfile(os.path.join(model_dir, cfg["gpt_checkpoint"])):
            files["gpt"] = load_gpt_checkpoint(os.path.join(model_dir, cfg["gpt_checkpoint"]))
        if files["bigvgan"] is None:
            # `BigVGAN.from_pretrained(cfg.vocoder.name)` (infer_v2.py:154-158, bigvgan.py:436-479) resolves a LOCAL directory holding
            # config.json + bigvgan_generator.pt (or the checkpoint file itself); a hub name is never fetched
            voc = str((cfg.get("vocoder") or {}).get("name", ""))
            cands = [os.path.join(model_dir, voc, "bigvgan_generator.pt"), os.path.join(voc, "bigvgan_generator.pt"), os.path.join(model_dir, voc),
                     os.path.join(model_dir, "bigvgan_generator.pt")]
            for p in cands:
                if voc or p == cands[-1]:
                    if os.path.isfile(p):
                        files["bigvgan"] = load_bigvgan_checkpoint(p)
                        cj = os.path.join(os.path.dirname(p), "config.json")
                        if derive_bcfg and os.path.isfile(cj):
                            import json

                            h = json.load(open(cj))
                            tup = lambda v: tuple(tup(x) for x in v) if isinstance(v, list) else v
                            bcfg.update({k: tup(v) for k, v in h.items() if k in bcfg})
                        break
        if files["codec"] is None and have("semantic_codec", "model.safetensors"):
            from safetensors.torch import load_file

            files["codec"] = load_file(os.path.join(model_dir, "semantic_codec", "model.safetensors"))
        if files["s2mel"] is None and cfg.get("s2mel_checkpoint") and have(cfg["s2mel_checkpoint"]):
            files["s2mel"] = load_s2mel_checkpoint(os.path.join(model_dir, cfg["s2mel_checkpoint"]))
        if files["campplus"] is None and have("campplus_cn_common.bin"):
            files["campplus"] = torch.load(os.path.join(model_dir, "campplus_cn_common.bin"), map_location="cpu", weights_only=True)
        for key in ("emo_matrix", "spk_matrix"):
            if files[key] is None and cfg.get(key) and have(cfg[key]):
                files[key] = torch.load(os.path.join(model_dir, cfg[key]), map_location="cpu", weights_only=True)
        return files, bcfg

    def _exchange_glue(self, files, bcfg, peer):
        """One packed RCCL message with every tensor that is not part of the two device arenas: the non-trunk tensors of gpt.pth
        (text tables, speed embedding, conditioning encoders), s2mel, the semantic codec, CAM++, the emotion matrices -- plus the
        small facts a receiver cannot derive without the files (BigVGAN's config, which dicts exist)."""
        from . import sharding
        from .gpt_engine import GPT_TENSOR_PREFIXES

        pack, meta = None, None
        if not peer:
            pack = {}
            for name in ("gpt", "bigvgan", "s2mel", "codec", "campplus"):
                sd = files[name]
                if sd is None:
                    continue
                for k, v in sd.items():
                    if name == "gpt" and k.startswith(GPT_TENSOR_PREFIXES):
                        continue  # the trunk travels as the packed device arena
                    if name == "bigvgan" and k != "conv_pre.weight":
                        continue  # (only its width is needed by the receiver's constructor; the weights travel as the arena)
                    if torch.is_tensor(v) and v.is_floating_point():
                        pack[f"{name}/{k}"] = v
            for name in ("emo_matrix", "spk_matrix"):
                if files[name] is not None:
                    pack[name] = files[name]
            meta = dict(bcfg=bcfg, present=[k for k, v in files.items() if v is not None])
        recv, meta = sharding.broadcast_state_dict(pack, self.device, src=0, meta=meta)
        if peer:
            out = {k: None for k in files}
            for name in meta["present"]:
                out[name] = {} if name in ("gpt", "bigvgan", "s2mel", "codec", "campplus") else None
            for k, v in recv.items():
                if "/" in k:
                    name, key = k.split("/", 1)
                    out[name][key] = v
                else:
                    out[k] = v
            return out, meta["bcfg"]
        return files, bcfg

    # ------------------------------------------------------------------ helpers mirrored from the reference
    def interval_silence(self, wavs, sampling_rate=22050, interval_silence=200):
        if not wavs or interval_silence <= 0:
            return wavs
        return torch.zeros(wavs[0].size(0), int(sampling_rate * interval_silence / 1000.0))

    def insert_interval_silence(self, wavs, sampling_rate=22050, interval_silence=200):
        if not wavs or interval_silence <= 0:
            return wavs
        sil = torch.zeros(wavs[0].size(0), int(sampling_rate * interval_silence / 1000.0))
        out = []
        for i, w in enumerate(wavs):
            out.append(w)
            if i < len(wavs) - 1:
                out.append(sil)
        return out

    def _prepare_gpt_inputs(self, conds_latent, text_ids):
        """-> fake ids [1, P], embeds [1, P-1, D], mask [1, P] (model_v2.py:598-661; one implementation: pipeline.prepare_gpt_inputs)."""
        embeds, pad, P = prepare_gpt_inputs(self.gpt_cfg, self.text_embedding, self.text_pos_embedding, conds_latent, text_ids)
        mask = torch.ones(1, P, dtype=torch.long, device=self.device)
        mask[0, :pad] = 0
        fake = torch.ones(1, P, dtype=torch.long, device=self.device)
        fake[0, -1] = self.gpt_cfg["start_mel_token"]
        return fake, embeds.unsqueeze(0), mask

    # ---- the once-per-prompt stages: an injected glue method wins, else the built-in prompt encoder, else a clear error
    def _stage(self, name, builtin):
        fn = getattr(self.glue, name, None) if self.glue is not None else None
        if fn is not None and getattr(type(self.glue), name, None) is not getattr(Glue, name, None):
            return fn
        if builtin is None:
            raise NotImplementedError(
                f"IndexTTS2.infer: stage '{name}' has no weights (missing under model_dir: {', '.join(self.missing_glue) or 'emotion matrices'}) "
                f"and no glue= override was given; nothing is downloaded or faked (INTEGRATION.md lists the model_dir layout)")
        return builtin

    def ready(self):
        """True when infer() can synthesise from audio: every stage has weights or an injected override."""
        try:
            self._stage("speaker", self.prompt.speaker if self.prompt else None)
            self._stage("emotion", self.prompt.emotion if self.prompt else None)
            if self.tokenizer is None:
                self._stage("tokenize", None)
            if self.s2mel is None:
                self._stage("s2mel", None)
            if self.cond is None:
                self._stage("merge_emovec", None)
        except NotImplementedError:
            return False
        return True

    def warm_up(self, seconds=3.0, text="Hello, hello. One, two, three."):
        """One synthetic request through EVERY stage (prompt side included) before the worker reports healthy: whatever a fresh
        process pays once -- the BLAS library's code objects for the shapes of this model, the 8-step decode graphs, the
        allocator's pools -- is paid here, at load, not by the first caller (the driver's fresh box spent 182 s in the first
        request of r02; the reference's lifespan loads the model and serves the first request cold, server.py:28-77).  A tone +
        noise prompt of `seconds` s at 22.05 kHz, a short text, at most 48 codes; the prompt caches are cleared afterwards.
        Returns the wall time, or None when the model cannot synthesise (missing stages) or the attempt failed."""
        import io as _io

        if not self.ready():
            return None
        t0 = time.perf_counter()
        rng = np.random.RandomState(0)
        t = np.arange(int(seconds * 22050)) / 22050.0
        x = 0.3 * np.sin(2 * np.pi * 140 * t) + 0.15 * np.sin(2 * np.pi * 280 * t + 1) + 0.02 * rng.randn(t.size)
        buf = _io.BytesIO()
        with wave.open(buf, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(22050)
            f.writeframes((np.clip(x, -1, 1) * np.iinfo(np.int16).max).astype("<i2").tobytes())
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                self.infer(buf.getvalue(), text, None, max_mel_tokens=48)
        except Exception as e:  # a warm-up must never keep a worker from starting
            logger.warning(f"warm-up request failed: {e}")
            return None
        finally:
            self.cache_spk_audio_prompt = self.cache_spk = self.cache_emo_audio_prompt = self.cache_emo_cond = None
        dt = time.perf_counter() - t0
        logger.info(f"warm-up request: {dt:.2f} seconds")
        return dt

    def _builtin_emo_mix(self, emo_vector, style, use_random):
        from .prompt import emo_vector_mix

        if self.emo_matrix is None or self.spk_matrix is None:
            return None
        return emo_vector_mix(emo_vector, style, self.emo_matrix, self.spk_matrix, self.emo_num, use_random)

    # ------------------------------------------------------------------ decode engines beside `self.gpt` (infer_many, beam groups)
    def _many_engine(self, slots):
        """A second decode engine whose slots are shared by the segments of several requests (wide MFMA GEMVs above 4 slots,
        on the bf16, fp16 or fp32 matrix cores by the model's GPT weight type: up to 32 slots for the 16-bit types, 16 for fp32)."""
        from . import _lib

        slots = max(1, min(int(slots), _lib.max_batch_for(self.gpt_dtype)))
        if slots not in self._engines:
            # a second engine SHAPE over the same device weights (ixtts_gpt_share_arena): it costs its KV cache only
            eng = GptEngine(self.gpt_cfg, dtype=self.gpt_dtype, max_seq=self.gpt.max_seq, max_batch=slots, device=self.device)
            self._engines[slots] = eng.share_arena(self.gpt)
        return self._engines[slots]

    def _beam_group_engine(self, num_beams, n_segments):
        """The engine several beam groups step together on: wide (5..32 slots on the matrix cores for a bf16 or fp16 model, 5..16
        for an fp32 one) when there is more than one segment to decode, else None (one group at a time on the register engine, as the
        reference decodes: segment after segment).  `IXTTS_BEAM_GROUPS` caps the groups (0 / 1: off); a bf16 or fp16 model defaults to 5,
        an fp32 model joins the groups only when the variable is set."""
        from . import _lib

        cap = int(os.environ.get("IXTTS_BEAM_GROUPS", "5"))
        most = _lib.max_batch_for(self.gpt_dtype) // num_beams  # 10 groups of 3 beams on a 16-bit model, 5 on an fp32 one
        groups = min(cap, most, n_segments)
        # An fp32 model takes this path only when IXTTS_BEAM_GROUPS is set explicitly: the fp32 wide step has no recorded timing
        # against the register engine yet, and the second engine's fp32 K/V cache is 8 GB at max_seq 2048.
        if self.gpt_dtype == "f32" and "IXTTS_BEAM_GROUPS" not in os.environ:
            return None
        if groups < 2 or groups * num_beams <= 4:
            return None
        want = min(cap, most) * num_beams  # one engine shape per worker, whatever the request's segment count
        eng = self._many_engine(want)
        return eng if eng.max_batch >= 2 * num_beams else None

    def _check_codes(self, codes):
        """The reference would index the semantic codec's codebook out of range with such a code (a device-side assert on a
        GPU, which takes the worker's context with it): refuse on the host instead."""
        if self.s2mel is not None and codes.numel():
            rows = self.s2mel.W["quantizer.codebook.weight"].shape[0]
            top = int(codes.max())
            if top >= rows:
                raise ValueError(f"mel code {top} outside the semantic codec's codebook ({rows} entries)")

    def _emo_text_vectors(self, requests, failed):
        """{request index: emo_vector} for the requests with `use_emo_text`: the emotion texts of the batch (`emo_text`, else the
        request's `text`) go through the Qwen emotion model together.  A failure lands in `failed` under the request's index."""
        want = {}
        for ri, rq in enumerate(requests):
            if not rq.get("use_emo_text"):
                continue
            if self.qwen_emo is None:
                failed[ri] = self._no_qwen_emo()
                continue
            try:
                want[ri] = rq["emo_text"] if rq.get("emo_text") is not None else rq["text"]
            except Exception as e:  # a request without `text`
                failed[ri] = e
        if not want:
            return {}
        texts = list(want.values())
        many = getattr(self.qwen_emo, "inference_many", None)
        try:
            dicts = many(texts) if many is not None else [self.qwen_emo.inference(t) for t in texts]
        except Exception as e:
            for ri in want:
                failed[ri] = e
            return {}
        logger.info(f"detected emotion vectors from text: {dicts}")
        return {ri: list(d.values()) for ri, d in zip(want, dicts)}

    # ------------------------------------------------------------------ the request path: every step once, for infer and infer_many
    def _generation_args(self, generation_kwargs):
        """Generation kwargs and their defaults (infer_v2.py:598-606) -> (namespace of the parsed values, the kwargs left over);
        do_sample is popped and then forced True (:648).  `typical_mass` and `seed` are read for the schedulers and stay among the
        leftovers, which `infer` forwards to `gpt.generate`; so do the constraint keywords, which `_generation_constraints` parses."""
        rest = dict(generation_kwargs)
        rest.pop("do_sample", True)
        g = SimpleNamespace(top_p=rest.pop("top_p", 0.8), top_k=rest.pop("top_k", 30), temperature=rest.pop("temperature", 0.8),
                            num_beams=rest.pop("num_beams", 3), length_penalty=rest.pop("length_penalty", 0.0),
                            repetition_penalty=rest.pop("repetition_penalty", 10.0), max_mel_tokens=rest.pop("max_mel_tokens", 1500),
                            typical_mass=float(rest.get("typical_mass", 0.9)) if rest.get("typical_sampling") else 0.0,
                            seed=int(rest.get("seed", 0)))
        return g, rest

    def _generation_constraints(self, rest):
        """The constraint keywords of HF `generate()` among the leftovers of `_generation_args` -- `min_new_tokens`, `min_length`,
        `no_repeat_ngram_size`, `suppress_tokens`, `begin_suppress_tokens`, `min_p` -- for the segments the schedulers decode ->
        (cfg, bans) or None when none is set: `cfg` under the engine's keyword names (`Segment.sampler`; a `min_length` stays under
        its own name until `_segment` knows the segment's prompt length: min_new_tokens = max(0, min_length - P), and
        `min_new_tokens` wins over it), `bans` = (suppress_tokens, begin_suppress_tokens) or None (`Segment.bans`).  `rest` is left
        alone: `gpt.generate` parses the same keywords itself.  A value the engine would refuse raises ValueError here, where it
        fails its own request only."""
        from . import _lib

        cfg, bans = generation_constraints(dict(rest))
        if cfg.get("min_new_tokens", 0) < 0:
            raise ValueError(f"generation: min_new_tokens {cfg['min_new_tokens']} is negative")
        if not 0 <= cfg.get("no_repeat_ngram_size", 0) <= _lib.NGRAM_MAX:
            raise ValueError(f"generation: no_repeat_ngram_size {cfg['no_repeat_ngram_size']} outside 0..{_lib.NGRAM_MAX}")
        if not 0.0 <= cfg.get("min_p", 0.0) <= 1.0:
            raise ValueError(f"generation: min_p {cfg['min_p']} outside 0..1")
        V = int(self.gpt_cfg["number_mel_codes"])
        for t in (bans or ((), ()))[0] + (bans or ((), ()))[1]:
            if not 0 <= t < V:
                raise ValueError(f"generation: suppressed id {t} outside 0..{V - 1}")
        return (cfg, bans) if cfg or bans is not None else None

    def _generation_processors(self, kwargs):
        """The other processor keywords of HF `generate()` among `kwargs` (a call's generation kwargs, a request's merged ones or
        the leftovers of `_generation_args`; left alone) -- `sequence_bias`, `bad_words_ids`, `forced_eos_token_id`,
        `exponential_decay_length_penalty`, `epsilon_cutoff`, `eta_cutoff`, `renormalize_logits` -- for the segments the schedulers
        decode -> (cfg, state) as `gpt_engine.generation_processors` returns them, or None when none is set: `cfg` joins
        `Segment.sampler`, `state` (the table of biased sequences and the forced ids) becomes `Segment.processors`; the step the
        forced ids are forced at is each segment's own `max_new` (`_segment`).  A bad value raises ValueError here, where it fails
        its own request only."""
        cfg, state = generation_processors(dict(kwargs), int(self.gpt_cfg["stop_mel_token"]), int(self.gpt_cfg["number_mel_codes"]))
        return (cfg, state) if cfg or state is not None else None

    def _no_qwen_emo(self):
        return NotImplementedError(
            f"use_emo_text needs the Qwen emotion model: no directory at model_dir/qwen_emo_path "
            f"({self.qwen_emo_dir or 'config.yaml names no qwen_emo_path'}); pass qwen_emo=... or provide it")

    @staticmethod
    def _resolve_emotion(emo_audio_prompt, emo_alpha, emo_vector):
        """infer_v2.py:476-505 -> (emo_prompt, emo_alpha, emo_vector, emo_is_spk): a vector takes the emotion prompt's place and is
        scaled by the clamped alpha (truncated to four decimals); without an emotion prompt the speaker prompt stands in at alpha
        1.0 (`emo_is_spk`)."""
        if emo_vector is not None:
            emo_audio_prompt = None
            scale = max(0.0, min(1.0, emo_alpha))
            if scale != 1.0:
                emo_vector = [int(x * scale * 10000) / 10000 for x in emo_vector]
        emo_is_spk = emo_audio_prompt is None
        return emo_audio_prompt, 1.0 if emo_is_spk else emo_alpha, emo_vector, emo_is_spk

    def _prompt_stages(self):
        return (self._stage("speaker", self.prompt.speaker if self.prompt else None),
                self._stage("emotion", self.prompt.emotion if self.prompt else None))

    def _encode_prompts(self, spk_prompt, emo_prompt):
        """-> (speaker dict, emotion features) through the prompt caches (infer_v2.py:508-580); no emotion prompt: the speaker's.
        A failing encode leaves no stale pair behind: the next request with the earlier prompt encodes it again."""
        speaker_fn, emotion_fn = self._prompt_stages()
        if emo_prompt is None:
            emo_prompt = spk_prompt
        if self.cache_spk is None or not _same_prompt(self.cache_spk_audio_prompt, spk_prompt):
            self.cache_spk, self.cache_spk_audio_prompt = None, None
            self.cache_spk, self.cache_spk_audio_prompt = speaker_fn(spk_prompt), spk_prompt
        if self.cache_emo_cond is None or not _same_prompt(self.cache_emo_audio_prompt, emo_prompt):
            self.cache_emo_cond, self.cache_emo_audio_prompt = None, None
            self.cache_emo_cond, self.cache_emo_audio_prompt = emotion_fn(emo_prompt), emo_prompt
        return self.cache_spk, self.cache_emo_cond

    def _conds_latent(self, spk, emo_cond, emo_is_spk, emo_alpha, emo_vector, use_random):
        """-> conds_latent [34, D], a function of the request's prompts only: computed once per request (the reference recomputes it
        per segment, infer_v2.py:629-635, model_v2.py:684-696 -- same values).  `emo_is_spk`: the built-in encoder takes the speaker's
        features for the emotion's too, one emotion-encoder pass instead of two."""
        if self.cond is not None:
            cond32, emovec = self.cond.encode_prompt(spk["spk_cond_emb"], None if emo_is_spk else emo_cond, emo_alpha)
        else:
            emovec = self._stage("merge_emovec", None)(spk["spk_cond_emb"], emo_cond, emo_alpha)
            cond32 = self._stage("get_conditioning", None)(spk["spk_cond_emb"])
        if emo_vector is not None:  # infer_v2.py:552-563,637-638
            mix = self._stage("emo_vector_mix", (lambda v, st, r: self._builtin_emo_mix(v, st, r)) if self.emo_matrix is not None else None)
            emovec_mat, weight_sum = mix(emo_vector, spk["style"], use_random)
            emovec = emovec_mat + (1 - weight_sum) * emovec
        return conds_latent(cond32, emovec, self.speed_emb)

    def _segments_of(self, text, max_text_tokens_per_segment, quick_streaming_tokens=0):
        """-> the text's segments as lists of token ids (infer_v2.py:582-589,617)."""
        if self.tokenizer is None:
            return self._stage("tokenize", None)(text, max_text_tokens_per_segment, quick_streaming_tokens)
        text_tokens_list = self.tokenizer.tokenize(text)
        text_token_ids = self.tokenizer.convert_tokens_to_ids(text_tokens_list)
        unk = self.tokenizer.unk_token_id
        if unk in text_token_ids:
            logger.warning(f"Input text contains {text_token_ids.count(unk)} unknown tokens (id={unk})")
            logger.warning(f"Tokens which can't be encoded: {[t for t, i in zip(text_tokens_list, text_token_ids) if i == unk]}")
        return [self.tokenizer.convert_tokens_to_ids(sent) for sent in
                self.tokenizer.split_segments(text_tokens_list, max_text_tokens_per_segment, quick_streaming_tokens=quick_streaming_tokens)]

    def _segment(self, conds_latent, ids, engine, max_mel_tokens, request=0, index=0, payload=None, stream=None, sampler=None, constraints=None,
                 processors=None):
        """One segment's text ids -> what the schedulers decode; `max_new` is taken against the engine that will decode it.
        `constraints`: what `_generation_constraints` returned -- its scalars join the segment's sampler settings (a sampler of its
        own only when there is something to set), its id lists become the segment's bans.  `processors`: what
        `_generation_processors` returned, likewise -- and forced eos ids are forced at this segment's own cap,
        `forced_eos_step = max_new` (ForcedEOSTokenLogitsProcessor's max_length = P + max_new)."""
        embeds, n_pad, P = prepare_gpt_inputs(self.gpt_cfg, self.text_embedding, self.text_pos_embedding, conds_latent, ids)
        max_new = max(0, min(max_mel_tokens, engine.max_seq - P - 2, self.gpt_cfg["max_mel_tokens"] - 1))
        bans = None
        if constraints is not None:
            cfg = resolve_min_length(constraints[0], P)
            if cfg:
                sampler = {**(sampler or {}), **cfg}
            bans = constraints[1]
        state = None
        if processors is not None:
            cfg, state = processors
            if state is not None and state["forced_eos"] and max_new >= 1:
                cfg = {**cfg, "forced_eos_step": max_new}
            if cfg:
                sampler = {**(sampler or {}), **cfg}
        return decode_segment(index, embeds, n_pad, max_new, request, payload, stream, sampler, bans, state)

    # what a request's `generation` dict may hold (infer_many): `infer`'s generation kwargs, parsed by `_generation_args`
    GENERATION_KEYS = ("top_p", "top_k", "temperature", "repetition_penalty", "length_penalty", "max_mel_tokens", "typical_sampling",
                       "typical_mass", "seed", "num_beams", "min_new_tokens", "min_length", "no_repeat_ngram_size", "suppress_tokens",
                       "begin_suppress_tokens", "min_p", "sequence_bias", "bad_words_ids", "forced_eos_token_id",
                       "exponential_decay_length_penalty", "epsilon_cutoff", "eta_cutoff", "renormalize_logits")

    def _request_generation(self, rq, generation_kwargs, g):
        """-> (generation namespace of this request, pinned, its constraints): a request with a `generation` dict overrides the
        call's kwargs with it and is PINNED -- its settings, seed and random streams are its own; one without it takes the call's
        (`g`).  The constraints are `_generation_constraints` of the same merged kwargs."""
        if "generation" not in rq:
            return g, False, self._generation_constraints(self._generation_args(generation_kwargs)[1])
        gen = dict(rq["generation"] or {})
        for k in gen:
            if k not in self.GENERATION_KEYS:
                raise ValueError(f"generation: unknown key {k!r} (known: {', '.join(self.GENERATION_KEYS)})")
        gr, rest = self._generation_args({**generation_kwargs, **gen})
        gr.num_beams = int(gr.num_beams)
        if gr.num_beams < 1:
            raise ValueError(f"generation: num_beams {gr.num_beams}")
        if gr.num_beams > 1 and not (2 <= gr.num_beams <= 4 and 1 <= gr.top_k <= 128):
            raise NotImplementedError("beam-sample on the device: 2 <= num_beams <= 4, 1 <= top_k <= 128")
        return gr, True, self._generation_constraints(rest)

    @staticmethod
    def _segment_sampler(g):
        """The namespace's settings under the keyword names the engine's decode() / beam_decode() take (`scheduler.Segment.sampler`)."""
        s = dict(repetition_penalty=g.repetition_penalty, temperature=g.temperature, top_k=g.top_k, top_p=g.top_p, seed=g.seed,
                 typical_mass=g.typical_mass)
        if g.num_beams > 1:
            s["length_penalty"] = g.length_penalty
        else:
            s["do_sample"] = g.top_k != 1
        return s

    def _many_engine_for(self, num_beams, decode_slots):
        """The engine `infer_many` decodes a `num_beams` class on: floor(decode_slots / num_beams) groups (the register engine up
        to 4 slots), or `decode_slots` single slots."""
        from . import _lib

        if num_beams > 1:
            groups = max(1, min(int(decode_slots), _lib.max_batch_for(self.gpt_dtype)) // num_beams)
            return self._many_engine(groups * num_beams) if groups * num_beams > 4 else self.gpt
        return self._many_engine(decode_slots)

    def _pinned_noise(self, item, seed, index, frames=None):
        """The CFM noise [1, in_channels, T] of segment `index` of a pinned request: drawn from (seed, index) alone, not from the
        process-wide generator whose state depends on what was served before.  `frames`: the segment's frame count under a speed
        or a fitted duration (None: `target_frames` of its codes)."""
        codes, pc = item[1], item[2]
        T = pc.shape[1] + (target_frames(codes.shape[-1]) if frames is None else int(frames))
        gen = torch.Generator(device=self.device).manual_seed((int(seed) * 1000003 + int(index)) & 0x7FFFFFFFFFFFFFFF)
        return torch.randn(1, self.s2mel.cfg["in_channels"], T, device=self.device, generator=gen)

    def _decode(self, engine, todo, g):
        """The segments through the engine's slots, weights read once per step for all of them -> {(request, index): ids}: beam
        groups when `g.num_beams > 1`, else one slot per segment (argmax when `top_k == 1`; with sampling each slot draws from its
        own counter-based stream)."""
        from .scheduler import BeamGroupScheduler, DecodeScheduler

        out = {}
        sampler = dict(repetition_penalty=g.repetition_penalty, temperature=g.temperature, top_k=g.top_k, top_p=g.top_p, seed=g.seed,
                       typical_mass=g.typical_mass)
        if todo and g.num_beams > 1:
            BeamGroupScheduler(engine, g.num_beams, batch_prefill=getattr(self, "prefill_batch", None)).run(todo, lambda seg, ids, score: out.__setitem__((seg.request, seg.index), ids),
                                                        length_penalty=g.length_penalty, **sampler)
        elif todo:
            DecodeScheduler(engine, engine.max_batch, self.stop_mel_token, batch_prefill=getattr(self, "prefill_batch", None)).run(
                todo, lambda seg, ids: out.__setitem__((seg.request, seg.index), ids), do_sample=g.top_k != 1, **sampler)
        torch.cuda.synchronize(self.device)
        return out

    def _trim_codes(self, ids):
        """-> codes [1, n] (int64, on the device): cut at the first stop token (infer_v2.py:676-687)."""
        row = (ids if torch.is_tensor(ids) else torch.from_numpy(np.asarray(ids).astype(np.int64))).to(self.device).reshape(-1)
        stops = (row == self.stop_mel_token).nonzero(as_tuple=False)
        n = int(stops[0]) if stops.numel() else row.numel()
        return row[:n].reshape(1, -1)

    def _latent_batching(self):
        """Whether a call's latents go through one `gpt.latent_many`: IXTTS_LATENT_BATCH as resolved, an engine that has the method
        (as the schedulers ask for `prefill_many`), and a `gpt.latent` that is the engine's own.  A `latent` replaced on the engine
        object -- a recorder or a third-party wrapper around the per-segment call -- keeps getting one call per segment: the packed
        call would go round it."""
        return bool(getattr(self, "latent_batch", False)) and hasattr(self.gpt, "latent_many") and "latent" not in vars(self.gpt)

    def _latent_entry(self, conds_latent, text_ids, codes):
        """-> (prefix [34 + L + 2, D], codes [n]), what `gpt.latent` / one entry of `gpt.latent_many` takes; refused on the host when a
        code lies outside the codebook."""
        self._check_codes(codes)
        return latent_prefix(self.gpt_cfg, self.text_embedding, self.text_pos_embedding, conds_latent, text_ids), codes[0]

    def _s2mel_item(self, conds_latent, text_ids, codes, spk, latent=None):
        """-> (latent [1, n, D], codes, prompt_condition, ref_mel, style): the latent pass (UnifiedVoice.forward, model_v2.py:554-596)
        over [conds; text] and the codes, refused on the host when a code lies outside the codebook.  `latent` [n, D]: the pass has
        run already (one `latent_many` for several segments)."""
        if latent is None:
            latent = self.gpt.latent(*self._latent_entry(conds_latent, text_ids, codes))
        return latent.unsqueeze(0), codes, spk["prompt_condition"], spk["ref_mel"], spk["style"]

    def _mels(self, items, spk, packed=False, noises=None, frames=None):
        """s2mel items -> one mel [1, 80, F] each (infer_v2.py:713-731): segment after segment through the built-in or the injected
        stage (which gets the speaker dict `spk`), or -- `packed`, IXTTS_S2MEL_BATCH=1 -- as ONE packed solve (S2Mel.solve_many).
        `noises`: per item the CFM noise of the built-in stage, or None for a draw from the default generator.  `frames`: per item
        the frame count of the built-in stage under a speed or a fitted duration (None, also for the whole list: the natural one)."""
        if packed:
            kw = {} if frames is None or all(f is None for f in frames) else dict(frames=frames)
            return self.s2mel.solve_many(items, n_timesteps=25, inference_cfg_rate=0.7, noises=noises, **kw)
        mels = []
        for i, (latent, codes, pc, rm, st) in enumerate(items):
            lens = torch.tensor([codes.shape[1]], dtype=torch.long, device=self.device)
            if self.s2mel is not None:
                kw = {} if frames is None or frames[i] is None else dict(frames=frames[i])
                mels.append(self.s2mel(latent, codes, lens, pc, rm, st, n_timesteps=25, inference_cfg_rate=0.7,
                                       noise=None if noises is None else noises[i], **kw))
            else:
                mels.append(self._stage("s2mel", None)(latent, codes, lens, spk))
        return mels

    last_loudness = None  # the level report of the last call: see `infer` / `infer_many`

    @staticmethod
    def _output_spec(output_sample_rate=None, output_encoding=None, output_loudness=None, output_peak=None, output_peak_mode=None,
                     output_limiter=None, duration=None, stream_return=False):
        """-> what the call asks of the output stage (`output.OutputSpec.of`), None: nothing, the host path; ValueError for a value
        outside the accepted ones, and for an encoding, a level or a limit on a stream."""
        return _output.OutputSpec.of(output_sample_rate, output_encoding, output_loudness, output_peak, output_peak_mode, output_limiter,
                                     duration=duration is not None, stream=stream_return)

    last_duration = None  # the pace report of the last call: see `infer` / `infer_many`

    def _rate_control(self, speed, duration, stream_return=False):
        """-> (speed | None, duration | None) of a call that asks for a pace; ValueError for a value outside `s2mel.SPEED_RANGE`, a
        duration that is not a positive number, both together (a duration implies its speed) and a duration on a stream (the fit
        needs every segment's code count before the first mel); NotImplementedError when the s2mel stage is an injected one."""
        if speed is None and duration is None:
            return None, None
        if speed is not None and duration is not None:
            raise ValueError("speed and duration cannot be combined: a duration fixes the speaking rate itself")
        if duration is not None and stream_return:
            raise ValueError("duration cannot be combined with stream_return=True: the fit needs every segment's codes before the first mel")
        speed, duration = check_speed(speed), _output.check_duration(duration)
        if self.s2mel is None:
            raise NotImplementedError("speed / duration set the frame count of the built-in s2mel stage (`S2Mel`: s2mel_state_dict=... or "
                                      "model_dir/<s2mel_checkpoint>); an injected `Glue.s2mel` has no such argument")
        return speed, duration

    @staticmethod
    def _paced_frames(items, speed=None, duration=None, rate=22050, interval_silence=200):
        """s2mel items -> (natural frame counts, the frame counts to ask for | None, delivered samples | None): `target_frames` at
        `speed`, or the fit of `duration` seconds at `rate` (`output.fit_frames`; DurationError when the range cannot reach it)."""
        natural = [target_frames(it[1].shape[1]) for it in items]
        if not items:
            return natural, None, None
        if duration is not None:
            frames, total, _ = _output.fit_frames(natural, duration, rate, interval_silence)
            return natural, frames, total
        if speed is not None:
            return natural, [target_frames(it[1].shape[1], speed) for it in items], None
        return natural, None, None

    @staticmethod
    def _duration_report(natural, frames, rate, interval_silence, delivered):
        """-> dict(natural_s, delivered_s, speed, pad_samples): the programme at its natural pace and as delivered (seconds at the
        delivered rate, gaps included), the effective speed sum(natural) / sum(frames), the trailing samples of silence."""
        return dict(natural_s=_output.delivered_len(natural, rate, interval_silence) / float(rate), delivered_s=delivered / float(rate),
                    speed=sum(natural) / float(sum(frames)), pad_samples=int(delivered - _output.delivered_len(frames, rate, interval_silence)))

    # ------------------------------------------------------------------ API
    def infer(self, spk_audio_prompt, text, output_path, emo_audio_prompt=None, emo_alpha=1.0, emo_vector=None,
              use_emo_text=False, emo_text=None, use_random=False, interval_silence=200, verbose=False,
              max_text_tokens_per_segment=120, stream_return=False, more_segment_before=0, output_sample_rate=None,
              output_encoding=None, output_loudness=None, output_peak=None, speed=None, duration=None, output_peak_mode=None,
              output_limiter=None, **generation_kwargs):
        """`output_sample_rate` (one of `output.SAMPLE_RATES`) / `output_encoding` (`pcm_s16le`, `mulaw`, `alaw`): the output stage on
        the device (output.py) takes the place of the host-side cat and int16 cast -- the `(sr, pcm)` return, the file at
        `output_path` and `last_timing["audio_length"]` follow the requested rate; pcm is uint8 for the G.711 encodings.  With
        `stream_return=True` the yielded segments are the resampled fp32 rows and an encoding is refused (the stream yields floats,
        as the reference's does).  Both None: 22 050 Hz int16, as ever.

        `output_loudness` (target integrated loudness, LUFS in [-50, -5]) / `output_peak` (sample-peak ceiling, dBFS in [-20, 0];
        -1 beside a loudness target): the output stage measures the delivered programme (ITU-R BS.1770-4, gaps included) on the device
        and applies ONE gain before the conversion -- lowered, never limited, when the ceiling would be passed.  Either one routes
        the request through the output stage (22 050 Hz `pcm_s16le` when no format is asked) and is refused with
        `stream_return=True`.  Afterwards `last_loudness` is dict(measured_lufs | None, gain_db, peak_dbfs_in, target_met), or None
        when neither was given -- and then nothing changes anywhere.

        `output_peak_mode` ("sample", the default, or "true": `output_peak` is then read in dBTP and held against the 4x-oversampled
        true peak of BS.1770 Annex 2; it needs one of the other three controls) / `output_limiter` (a bool; True is a level control of
        its own, with a ceiling of -1 when `output_peak` is not given): with the limiter the loudness gain does not give way, and a
        look-ahead limiter on the device removes what exceeds the ceiling, sample by sample, so the ceiling no longer costs the
        programme its target.  Both are refused with `stream_return=True`.  A call with either gets more keys in `last_loudness`:
        peak_mode, limited, max_reduction_db, limited_fraction, delivered_lufs, delivered_peak_dbfs (`output.level_report_limit`).

        `speed` (speaking rate, a float in `s2mel.SPEED_RANGE` = [0.5, 2.0]): the length regulator stretches every segment's codes to
        `target_frames(n, speed)` mel frames -- tempo changes, pitch does not; the codes are those of any other speed.  `duration`
        (seconds of the whole delivered programme, gaps included, at the delivered rate): the frame counts are fitted once every
        segment's codes are known (`output.fit_frames`: proportional to the natural ones, the largest total that fits), and trailing
        silence fills the rest: exactly int(duration * rate + 0.5) samples leave, through the output stage (22 050 Hz `pcm_s16le`
        when no format is asked).  A duration whose implied speed leaves the range raises `output.DurationError` (a ValueError with
        `natural_s`, `min_s`, `max_s`).  The two are refused together, `duration` also with `stream_return=True`, and either with an
        injected `Glue.s2mel` (NotImplementedError).  Afterwards `last_duration` is dict(natural_s, delivered_s, speed, pad_samples),
        or None when neither was given -- and then nothing changes anywhere."""
        if speed is not None or duration is not None:
            self._rate_control(speed, duration, stream_return)
        # refused here, not at the generator's first step
        self._output_spec(output_sample_rate, output_encoding, output_loudness, output_peak, output_peak_mode, output_limiter, duration, stream_return)
        gen = self.infer_generator(spk_audio_prompt, text, output_path, emo_audio_prompt, emo_alpha, emo_vector, use_emo_text,
                                   emo_text, use_random, interval_silence, verbose, max_text_tokens_per_segment, stream_return,
                                   more_segment_before, output_sample_rate=output_sample_rate, output_encoding=output_encoding,
                                   output_loudness=output_loudness, output_peak=output_peak, speed=speed, duration=duration,
                                   output_peak_mode=output_peak_mode, output_limiter=output_limiter, **generation_kwargs)
        if stream_return:
            return gen
        try:
            return list(gen)[0]
        except IndexError:
            return None

    @torch.no_grad()
    def infer_many(self, requests, interval_silence=200, max_text_tokens_per_segment=120, decode_slots=8, output_sample_rate=None,
                   output_encoding=None, output_loudness=None, output_peak=None, speed=None, duration=None, output_peak_mode=None,
              output_limiter=None, **generation_kwargs):
        """Several `/tts` requests served TOGETHER (the worker's global lock, server.py:25,384, replaced by the
        decode scheduler): every request's segments share the decode slots -- the weights are read once per step for all of them
        -- and the post-decode stages run per segment as in `infer`, through the same helpers.  Each request is a dict with
        `spk_audio_prompt`, `text` and optionally `emo_audio_prompt`, `emo_alpha`, `emo_vector`, `use_random`, `use_emo_text`,
        `emo_text` (the emotion from text, as in `infer`; the emotion texts of the whole batch are decoded together).  Generation
        kwargs and defaults are `infer`'s: with `num_beams > 1` (the served default, 3) every segment is a beam GROUP and
        floor(decode_slots / num_beams) groups step together; `num_beams=1` samples without beams, one slot per segment (argmax
        when `top_k == 1`).  `decode_slots` goes up to 32 on a bf16 / fp16 model and up to 16 on an fp32 one (more is clamped).

        The constraint keywords of HF `generate()` -- `min_new_tokens`, `min_length`, `no_repeat_ngram_size`, `suppress_tokens`,
        `begin_suppress_tokens`, `min_p` -- and the processor keywords -- `sequence_bias`, `bad_words_ids`, `forced_eos_token_id`,
        `exponential_decay_length_penalty`, `epsilon_cutoff`, `eta_cutoff`, `renormalize_logits` -- hold for every segment of the call,
        as they do in `infer`.

        A request may carry `generation`, a dict with any of `GENERATION_KEYS` (top_p, top_k, temperature, repetition_penalty,
        length_penalty, max_mel_tokens, typical_sampling, typical_mass, seed, num_beams, the six constraint keywords and the seven processor keywords;
        `sequence_bias` in HF's list form [[[ids], bias], ...], which survives JSON): it overrides the call's kwargs for that
        request, and the request is PINNED (even with `{}`): segment i decodes under the request's settings and seed from random
        stream i, and the built-in s2mel's noise comes from (seed, i).  Its codes and PCM are then a function of the request
        alone -- bit-identical alone or in any batch, in any order -- on every wide engine (`decode_slots` 5..32: the bits are the
        same on all of them; only the register engines of up to 4 slots differ in logit bits) and outside IXTTS_S2MEL_BATCH=1 (the packed solve reassociates with its pack).
        `num_beams` may differ between requests: each value decodes as its own class, one after another.  An unknown key, or a
        `num_beams` the engine chosen for `decode_slots` cannot hold, fails that request only.  Requests without the key behave
        as ever: the call's settings, streams by slot / submission order, noise from the default generator.

        `output_sample_rate` / `output_encoding` (see `infer`) hold for the call; a request may carry its own `sample_rate` and
        `encoding` beside `generation` (they do not pin it).  The requests that ask for a format leave through the output stage on
        the device together (`output.finish_pcm_many`: one resample launch per distinct rate, one conversion launch per distinct
        encoding, one copy to the host), and a pinned request's bytes stay a function of the request alone; a value outside the
        accepted sets fails that request only.  The requests that ask for nothing take the host path they always took.

        `output_loudness` / `output_peak` (see `infer`) hold for the call as well, a request may carry `loudness` / `peak` (they do
        not pin it either, and a bad value fails that request only); a request with either leaves through the output stage.
        `last_loudness` is then a list with one entry per request: the level report, or None where no control was asked.
        `output_peak_mode` / `output_limiter` (see `infer`) likewise, with the request keys `peak_mode` / `limiter`.

        `speed` / `duration` (see `infer`) hold for the call; a request may carry its own `speed` or `duration` (then the call's pair
        does not apply to it; they do not pin it, and a bad value or a duration that cannot be met fails that request only).  The
        decode and the latent pass do not see them.  A request with a duration leaves through the output stage.  A pinned request
        with either keeps its guarantee also under IXTTS_S2MEL_BATCH=1: its segments are then packed among themselves, not with
        the rest of the batch.  `last_duration` is a list with one entry per request: the pace report, or None where neither was asked.

        Returns one entry per request: `(22050, int16 [N, 1])` (`(rate, int16 | uint8 [N, 1])` with a format), None (empty text), or the EXCEPTION that
        request raised (bad prompt audio, a code outside the codebook ...) -- one request's failure leaves the others of the
        batch alone."""
        g, _ = self._generation_args(generation_kwargs)
        g.num_beams = int(g.num_beams)
        self._prompt_stages()  # a model without prompt stages refuses the whole call
        if g.num_beams > 1 and not (2 <= g.num_beams <= 4 and 1 <= g.top_k <= 128):
            raise NotImplementedError("beam-sample on the device: 2 <= num_beams <= 4, 1 <= top_k <= 128")
        # segments decode per `num_beams` class (the call's, and whatever pinned requests ask for), each class on its own engine
        engines = {g.num_beams: self._many_engine_for(g.num_beams, decode_slots)}
        classes = {}  # num_beams -> segments
        start = time.perf_counter()
        plans = [None] * len(requests)
        failed = {}
        text_emo = self._emo_text_vectors(requests, failed)
        call_wide = dict(output_sample_rate=output_sample_rate, output_encoding=output_encoding, output_loudness=output_loudness,
                         output_peak=output_peak, output_peak_mode=output_peak_mode, output_limiter=output_limiter)
        for ri, rq in enumerate(requests):
            if ri in failed:
                continue
            try:
                spk_prompt = rq["spk_audio_prompt"]
                # infer_v2.py:475-488: the emotion from text takes the place of a given vector
                emo_prompt, emo_alpha, emo_vector, emo_is_spk = self._resolve_emotion(
                    rq.get("emo_audio_prompt"), rq.get("emo_alpha", 1.0), text_emo[ri] if ri in text_emo else rq.get("emo_vector"))
                spk, emo_cond = self._encode_prompts(spk_prompt, emo_prompt)
                cl = self._conds_latent(spk, emo_cond, emo_is_spk, emo_alpha, emo_vector, rq.get("use_random", False))
                segments = self._segments_of(rq["text"], max_text_tokens_per_segment)
                own = rq.get("speed") is not None or rq.get("duration") is not None  # the request's own pace, else the call's
                pace = self._rate_control(rq.get("speed") if own else speed, rq.get("duration") if own else duration)  # a bad value fails this request
                # what the request asks of the output stage: its own keys, else the call's; None = the host path (a bad value fails this request)
                spec = self._output_spec(**{kw: rq[key] if rq.get(key) is not None else call_wide[kw] for key, kw in _output.OUTPUT_KEYS},
                                         duration=pace[1])
                gr, pinned, cons = self._request_generation(rq, generation_kwargs, g)
                procs = self._generation_processors({**generation_kwargs, **(rq.get("generation") or {})})
                nb = gr.num_beams
                if nb not in engines:
                    engines[nb] = self._many_engine_for(nb, decode_slots)
                eng = engines[nb]
                if nb > 1 and eng.max_batch < nb:
                    raise NotImplementedError(f"num_beams={nb} needs {nb} decode slots: the engine chosen for decode_slots={decode_slots} holds {eng.max_batch}")
                # a pinned request: segment i under the request's own settings and seed, drawing from stream i
                sampler = self._segment_sampler(gr) if pinned else None
                mine = [self._segment(cl, ids, eng, gr.max_mel_tokens, request=ri, index=si, stream=si if pinned else None, sampler=sampler,
                                      constraints=cons, processors=procs)
                        for si, ids in enumerate(segments)]
                plans[ri] = dict(spk=spk, cl=cl, segments=segments, seed=gr.seed if pinned else None, spec=spec, pace=pace)
                classes.setdefault(nb, []).extend(mine)  # only once the whole request is known to be well-formed
            except Exception as e:  # this request only
                failed[ri] = e
        decoded, todo = {}, []
        for nb, segs in (classes or {g.num_beams: []}).items():
            # the run's settings (idle slots, parked groups, unpinned segments): the call's in its own class; another class holds
            # pinned segments only and idles under the served defaults
            gc = g if nb == g.num_beams else self._generation_args(dict(num_beams=nb))[0]
            decoded.update(self._decode(engines[nb], segs, gc))
            todo += segs
        t_decode = time.perf_counter() - start
        # per request: codes -> latents (a code outside the codebook fails its request only, before anything is packed); a segment
        # without codes is left out
        # IXTTS_LATENT_BATCH=1 (the default): the checks per request, then ONE `latent_many` over every surviving segment of every
        # request (packed passes over the weights, every latent the bits of its own `latent` call), the latents handed back to their
        # plans; should the packed call raise, the latents are redone segment by segment so that an exception lands on the request
        # that caused it (the rule of `vocode_many`)
        batch = self._latent_batching()
        for ri, plan in enumerate(plans):
            if ri in failed:
                continue
            try:
                codes = [self._trim_codes(decoded[ri, si]) for si in range(len(plan["segments"]))]
                plan["kept"] = kept = [si for si, c in enumerate(codes) if c.shape[1]]
                plan["codes"] = codes
                if batch:
                    plan["entries"] = [self._latent_entry(plan["cl"], plan["segments"][si], codes[si]) for si in kept]
                else:
                    plan["latents"] = [None] * len(kept)  # `_s2mel_item` runs the pass
            except Exception as e:  # this request only
                failed[ri] = e
        if batch:
            live = [ri for ri in range(len(plans)) if ri not in failed]
            try:
                lat = iter(self.gpt.latent_many([en for ri in live for en in plans[ri]["entries"]]))
                for ri in live:
                    plans[ri]["latents"] = [next(lat) for _ in plans[ri]["entries"]]
            except Exception:
                for ri in live:
                    plans[ri]["latents"] = [None] * len(plans[ri]["entries"])
        for ri, plan in enumerate(plans):
            if ri in failed:
                continue
            try:
                kept, codes = plan["kept"], plan["codes"]
                plan["items"] = [self._s2mel_item(plan["cl"], plan["segments"][si], codes[si], plan["spk"], latent=lt)
                                 for si, lt in zip(kept, plan["latents"])]
                # a pinned request's audio is a function of the request: the built-in s2mel's noise comes from its seed, per segment
                pin = plan["seed"] is not None and self.s2mel is not None
                plan["frames"] = None
                if plan["pace"] != (None, None):  # the frame counts under the request's speed, or fitted to its duration (which may refuse)
                    plan["rate"] = plan["spec"].rate if plan["spec"] is not None else 22050
                    plan["natural"], plan["frames"], plan["total"] = self._paced_frames(plan["items"], *plan["pace"], plan["rate"], interval_silence)
                    plan["noises"] = [self._pinned_noise(it, plan["seed"], si, fr) if pin else None
                                      for si, it, fr in zip(kept, plan["items"], plan["frames"])]
                    continue
                plan["noises"] = [self._pinned_noise(it, plan["seed"], si) if pin else None for si, it in zip(kept, plan["items"])]
            except Exception as e:  # this request only
                failed[ri] = e
        # s2mel, IXTTS_S2MEL_BATCH=1: every surviving segment of every request in one packed solve -- an exception raised inside it
        # is returned for every request of the batch; default, or an injected s2mel stage: segment after segment
        live = [ri for ri in range(len(plans)) if ri not in failed]
        if self.s2mel is not None and s2mel_batching():
            # a pinned request with a pace: a pack of its own, so that its bits stay a function of the request alone
            alone = [ri for ri in live if plans[ri]["frames"] is not None and plans[ri]["seed"] is not None]
            for ri in alone:
                try:
                    plans[ri]["mels"] = self._mels(plans[ri]["items"], None, packed=True, noises=plans[ri]["noises"], frames=plans[ri]["frames"])
                except Exception as e:  # this request only
                    failed[ri] = e
            live = [ri for ri in live if ri not in alone]
            try:
                if live or not alone:
                    frames = [f for ri in live for f in (plans[ri]["frames"] or [None] * len(plans[ri]["items"]))]
                    mels = iter(self._mels([it for ri in live for it in plans[ri]["items"]], None, packed=True,
                                           noises=[z for ri in live for z in plans[ri]["noises"]], frames=frames))
                    for ri in live:
                        plans[ri]["mels"] = [next(mels) for _ in plans[ri]["items"]]
            except Exception as e:
                for ri in live:
                    failed[ri] = e
        else:
            for ri in live:
                try:
                    plans[ri]["mels"] = self._mels(plans[ri]["items"], plans[ri]["spk"], noises=plans[ri]["noises"], frames=plans[ri]["frames"])
                except Exception as e:  # this request only
                    failed[ri] = e
        # vocoder: the mels of every surviving request in batched passes (`vocode_many`; IXTTS_BV_BATCH=0, or an injected vocoder:
        # mel after mel).  A mel that raises comes back as its exception and fails its own request only.
        live = [ri for ri in range(len(plans)) if ri not in failed]
        pcm = iter(vocode_many(self.bigvgan, [mel for ri in live for mel in plans[ri]["mels"]]))
        for ri in live:
            plans[ri]["pcm"] = [next(pcm) for _ in plans[ri]["mels"]]
        # the requests that ask something of the output stage: through it on the device, all of them together
        formatted = {}
        self.last_loudness = [None] * len(requests)
        mine = [ri for ri in live if plans[ri]["spec"] is not None and not any(isinstance(w, Exception) for w in plans[ri]["pcm"])]
        if mine:
            try:
                specs = [plans[ri]["spec"]._replace(total=plans[ri].get("total")) for ri in mine]  # (the sample count of a fitted duration)
                res, reports = _output.finish([plans[ri]["pcm"] for ri in mine], specs, interval_silence)
                for ri, rep in zip(mine, reports):
                    self.last_loudness[ri] = rep
                    if rep is not None:
                        logger.info(f"infer_many: request {ri} level: {rep}")
                formatted = dict(zip(mine, res))
            except Exception as e:
                formatted = {ri: e for ri in mine}
        out = []
        for ri, plan in enumerate(plans):
            if ri in failed:
                out.append(failed[ri])
                continue
            if ri in formatted:
                out.append(formatted[ri])
                continue
            try:
                for w in plan["pcm"]:
                    if isinstance(w, Exception):
                        raise w
                wavs = [w.cpu() for w in plan["pcm"]]
                if not wavs:
                    out.append(None)
                    continue
                wav = torch.cat(self.insert_interval_silence(wavs, sampling_rate=22050, interval_silence=interval_silence), dim=1)
                out.append((22050, wav.type(torch.int16).numpy().T))
            except Exception as e:  # this request only
                out.append(e)
        self.last_duration = [None] * len(requests)
        for ri, plan in enumerate(plans):
            if isinstance(out[ri], tuple) and plan.get("frames"):
                self.last_duration[ri] = self._duration_report(plan["natural"], plan["frames"], plan["rate"], interval_silence, out[ri][1].shape[0])
        total = time.perf_counter() - start
        audio = sum(o[1].shape[0] for o in out if isinstance(o, tuple)) / 22050.0
        if formatted:  # every result at its own rate
            audio = sum(o[1].shape[0] / float(o[0]) for o in out if isinstance(o, tuple))
        logger.info(f"infer_many: {len(requests)} requests ({sum(isinstance(o, Exception) for o in out)} failed), {len(todo)} segments, "
                    f"decode {t_decode:.2f} s, total {total:.2f} s, audio {audio:.2f} s, RTF {total / max(audio, 1e-9):.4f}")
        self.last_timing = dict(gpt_gen_time=t_decode, total=total, audio_length=audio)
        return out

    def infer_generator(self, spk_audio_prompt, text, output_path, emo_audio_prompt=None, emo_alpha=1.0, emo_vector=None,
                        use_emo_text=False, emo_text=None, use_random=False, interval_silence=200, verbose=False,
                        max_text_tokens_per_segment=120, stream_return=False, quick_streaming_tokens=0, output_sample_rate=None,
                        output_encoding=None, output_loudness=None, output_peak=None, speed=None, duration=None, output_peak_mode=None,
              output_limiter=None, **generation_kwargs):
        logger.info("Starting inference...")
        start_time = time.perf_counter()
        speed, duration = self._rate_control(speed, duration, stream_return)  # a pace (see `infer`); a duration leaves through the output stage too
        self.last_duration = None
        paced = []  # (natural, asked) frame counts per segment, for `last_duration`
        # an output format, a level or a duration (see `infer`): the segments stay on the device and leave through `output.finish`
        spec = self._output_spec(output_sample_rate, output_encoding, output_loudness, output_peak, output_peak_mode, output_limiter, duration,
                                 stream_return)
        self.last_loudness = None
        self._prompt_stages()
        gpt_gen_time = gpt_forward_time = s2mel_time = bigvgan_time = 0.0
        if use_emo_text:
            # infer_v2.py:475-488: the emotion reference clip gives way, the text (or `text`) becomes the emotion vector
            if self.qwen_emo is None:
                raise self._no_qwen_emo()
            q0 = time.perf_counter()
            emo_dict = self.qwen_emo.inference(text if emo_text is None else emo_text)
            gpt_gen_time += time.perf_counter() - q0  # the emotion decode counts as generation time (the reference books it under the total only)
            logger.info(f"detected emotion vectors from text: {emo_dict}")
            emo_vector = list(emo_dict.values())
        emo_prompt, emo_alpha, emo_vector, _ = self._resolve_emotion(emo_audio_prompt, emo_alpha, emo_vector)
        spk, emo_cond = self._encode_prompts(spk_audio_prompt, emo_prompt)
        segments = self._segments_of(text, max_text_tokens_per_segment, quick_streaming_tokens)
        g, rest = self._generation_args(generation_kwargs)
        sampling_rate = 22050
        m0 = time.perf_counter()
        # Without an emotion prompt `infer` still hands the encoder the emotion stage's own features of the speaker prompt (loaded at
        # 16 kHz, as the reference loads them: infer_v2.py:565-580) at alpha 1.0, where `infer_many` reuses the speaker's features
        # in one pass: the two differ in the last bits with the built-in prompt encoder, so `emo_is_spk` stays False here.
        cl = self._conds_latent(spk, emo_cond, False, emo_alpha, emo_vector, use_random)
        # Without beams the segments are independent sequences: decode them together, the weights are read once per step for
        # all of them (the reference decodes segment after segment, infer_v2.py:616; tokens per segment are the same for
        # greedy).  With beams every segment is a beam GROUP (its own scorer state, its own random stream: the segment index) and
        # the groups step together on the wide engine when `_beam_group_engine` gives one; else -- and for one segment, streaming
        # or a logits processor -- `gpt.generate`, one segment at a time.
        eng = None
        if len(segments) > 1 and not stream_return and not rest.get("logits_processor"):
            if g.num_beams == 1:
                eng = self.gpt
            elif g.num_beams > 1 and 1 <= g.top_k <= 128:
                eng = self._beam_group_engine(g.num_beams, len(segments))
        pre = None
        if eng is not None:
            beams = g.num_beams > 1
            cons = self._generation_constraints(rest)  # (the one-segment path below hands `rest` to gpt.generate, which parses them itself)
            procs = self._generation_processors(rest)
            pre = self._decode(eng, [self._segment(cl, ids, eng, g.max_mel_tokens, index=i, stream=i if beams else None, constraints=cons, processors=procs)
                                     for i, ids in enumerate(segments)], g)
        gpt_gen_time += time.perf_counter() - m0
        # several segments, whole audio at the end, IXTTS_S2MEL_BATCH=1: their CFM solves run as ONE packed solve (default: segment
        # after segment, as the reference); streaming keeps the per-segment order for its first-chunk latency
        pack_solve = not stream_return and len(segments) > 1 and self.s2mel is not None and s2mel_batching()
        packed = [] if pack_solve or duration is not None else None  # (a duration is fitted once every segment's codes are known)
        wavs, total = [], None  # (total: the samples a fitted duration delivers)
        has_warned = False
        silence = None
        # the segments were decoded up front, so every segment's codes are known: IXTTS_LATENT_BATCH=1 runs ONE `latent_many` for all of
        # them here and the loop takes its latents from the result (the same bits as its own `latent` call).  Anything this cannot
        # do -- a segment without codes, a code outside the codebook -- is left to the loop, which raises it where it always did.
        latents = trimmed = None
        if pre is not None and self._latent_batching():
            m0 = time.perf_counter()
            trimmed = [self._trim_codes(torch.from_numpy(np.asarray(pre[0, i]).astype(np.int64)).reshape(1, -1).to(self.device))
                       for i in range(len(segments))]  # (once per segment: the loop takes them from here)
            try:
                if all(c.shape[1] for c in trimmed):
                    latents = self.gpt.latent_many([self._latent_entry(cl, ids, c) for ids, c in zip(segments, trimmed)])
                    torch.cuda.synchronize(self.device)
            except Exception:
                latents = None
            gpt_forward_time += time.perf_counter() - m0
        for seg_index, sent_ids in enumerate(segments):
            m0 = time.perf_counter()
            if pre is not None:
                codes = torch.from_numpy(np.asarray(pre[0, seg_index]).astype(np.int64)).reshape(1, -1).to(self.device)
            else:
                fake, embeds, mask = self._prepare_gpt_inputs(cl, sent_ids)
                self.gpt.store_mel_emb(embeds)
                trunc = fake.shape[1]
                out = self.gpt.generate(fake, bos_token_id=self.gpt_cfg["start_mel_token"], pad_token_id=self.stop_mel_token,
                                        eos_token_id=self.stop_mel_token, attention_mask=mask, max_length=trunc + g.max_mel_tokens,
                                        num_return_sequences=1, do_sample=True, top_p=g.top_p, top_k=g.top_k, temperature=g.temperature,
                                        num_beams=g.num_beams, repetition_penalty=g.repetition_penalty, length_penalty=g.length_penalty,
                                        **rest)
                codes = out[:, trunc:]
                torch.cuda.synchronize(self.device)
                gpt_gen_time += time.perf_counter() - m0
            if codes.shape[1] == 0:  # no room left to generate (max_mel_tokens == 0 or a prompt as long as max_seq)
                raise RuntimeError(f"no mel codes could be generated for segment {seg_index} (max_mel_tokens={g.max_mel_tokens}, max_seq={self.gpt.max_seq})")
            if not has_warned and bool((codes[:, -1] != self.stop_mel_token).any()):
                warnings.warn(f"WARN: generation stopped due to exceeding `max_mel_tokens` ({g.max_mel_tokens}). "
                              f"Input text tokens: {len(sent_ids)}. Consider reducing `max_text_tokens_per_segment`"
                              f"({max_text_tokens_per_segment}) or increasing `max_mel_tokens`.", category=RuntimeWarning)
                has_warned = True
            m0 = time.perf_counter()
            item = self._s2mel_item(cl, sent_ids, self._trim_codes(codes) if trimmed is None else trimmed[seg_index], spk,
                                    latent=None if latents is None else latents[seg_index])
            torch.cuda.synchronize(self.device)
            gpt_forward_time += time.perf_counter() - m0
            if packed is not None:  # every segment's CFM in one solve after the loop
                packed.append(item)
                continue
            m0 = time.perf_counter()
            if speed is None:
                mel = self._mels([item], spk)[0]
            else:
                natural, frames, _ = self._paced_frames([item], speed)
                paced.append((natural[0], frames[0]))
                mel = self._mels([item], spk, frames=frames)[0]
            torch.cuda.synchronize(self.device)
            s2mel_time += time.perf_counter() - m0
            m0 = time.perf_counter()
            wav = vocode(self.bigvgan, mel)
            torch.cuda.synchronize(self.device)
            bigvgan_time += time.perf_counter() - m0
            if spec is not None:
                wavs.append(wav)
                if stream_return:  # the resampled, clamped fp32 row, and silence of the new length
                    yield (wav if spec.rate == sampling_rate else _output.Resampler(spec.rate, wav.device).forward_many([wav])[0]).cpu()
                    if silence is None:
                        silence = torch.zeros(wav.size(0), _output.gap_len(spec.rate, interval_silence))
                    yield silence
                continue
            wavs.append(wav.cpu())
            if stream_return:
                yield wav.cpu()
                if silence is None:
                    silence = self.interval_silence(wavs, sampling_rate=sampling_rate, interval_silence=interval_silence)
                yield silence
        if packed:
            m0 = time.perf_counter()
            if speed is None and duration is None:
                mels = self._mels(packed, spk, packed=True)
            else:
                natural, frames, total = self._paced_frames(packed, speed, duration, spec.rate if spec is not None else sampling_rate, interval_silence)
                paced = list(zip(natural, frames))
                mels = self._mels(packed, spk, packed=pack_solve, frames=frames)
            torch.cuda.synchronize(self.device)
            s2mel_time += time.perf_counter() - m0
            m0 = time.perf_counter()
            wavs = []
            for w in vocode_many(self.bigvgan, mels):  # one batched pass (IXTTS_BV_BATCH=0: mel after mel)
                if isinstance(w, Exception):
                    raise w
                wavs.append(w if spec is not None else w.cpu())  # (.cpu() waits for the vocoder)
            if spec is not None:
                torch.cuda.synchronize(self.device)
            bigvgan_time += time.perf_counter() - m0
        end_time = time.perf_counter()
        if not wavs:
            return
        if spec is not None:
            ((sampling_rate, pcm),), (self.last_loudness,) = _output.finish([wavs], [spec._replace(total=total)], interval_silence)
            if self.last_loudness is not None:
                logger.info(f"output level: {self.last_loudness}")
            wav_length = pcm.shape[0] / sampling_rate
            end_time = time.perf_counter()  # (the output stage is part of the request)
        else:
            wavs = self.insert_interval_silence(wavs, sampling_rate=sampling_rate, interval_silence=interval_silence)
            wav = torch.cat(wavs, dim=1)
            wav_length = wav.shape[-1] / sampling_rate
        if paced:
            self.last_duration = self._duration_report([a for a, _ in paced], [b for _, b in paced], sampling_rate, interval_silence,
                                                       int(round(wav_length * sampling_rate)))
            logger.info(f"pace: {self.last_duration}")
        logger.info(f"gpt_gen_time: {gpt_gen_time:.2f} seconds")
        logger.info(f"gpt_forward_time: {gpt_forward_time:.2f} seconds")
        logger.info(f"s2mel_time: {s2mel_time:.2f} seconds")
        logger.info(f"bigvgan_time: {bigvgan_time:.2f} seconds")
        logger.info(f"Total inference time: {end_time - start_time:.2f} seconds")
        logger.info(f"Generated audio length: {wav_length:.2f} seconds")
        logger.info(f"RTF: {(end_time - start_time) / wav_length:.4f}")
        self.last_timing = dict(gpt_gen_time=gpt_gen_time, gpt_forward_time=gpt_forward_time, s2mel_time=s2mel_time,
                                bigvgan_time=bigvgan_time, total=end_time - start_time, audio_length=wav_length)
        if spec is not None:
            if output_path:
                if os.path.isfile(output_path):
                    os.remove(output_path)
                if os.path.dirname(output_path) != "":
                    os.makedirs(os.path.dirname(output_path), exist_ok=True)
                with open(output_path, "wb") as f:
                    f.write(_output.wav_bytes(sampling_rate, pcm, spec.encoding))
            if not stream_return:
                yield output_path if output_path else (sampling_rate, pcm)
            return
        wav = wav.cpu()
        if output_path:
            if os.path.isfile(output_path):
                os.remove(output_path)
            if os.path.dirname(output_path) != "":
                os.makedirs(os.path.dirname(output_path), exist_ok=True)
            pcm = wav.type(torch.int16).numpy()  # truncation toward zero, as torchaudio.save(wav.type(torch.int16)) (infer_v2.py:772)
            with wave.open(output_path, "wb") as f:
                f.setnchannels(pcm.shape[0])
                f.setsampwidth(2)
                f.setframerate(sampling_rate)
                f.writeframes(pcm.T.astype("<i2").tobytes())
            if stream_return:
                return
            yield output_path
        else:
            if stream_return:
                return
            yield (sampling_rate, wav.type(torch.int16).numpy().T)
