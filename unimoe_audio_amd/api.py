"""High-level API surface of the reference, on the HIP engine.

Keeps both spellings the reference ships: the HF-directory flavour (`UniMoE_Audio.py:39-261`:
`text_to_speech(transcription, prompt_transcription, prompt_wav, output_dir, max_audio_seconds, ...)`) and the in-repo twin
(`utils/UniMoE_Audio_mod.py:294-619`: `caption`, `prompt_text`, `save_name`, `cfg_scale`, ...).  Prompt templates, negative /
positive prompt pairing and `max_tokens = 50 * seconds` follow the reference (mod.py:56-59,343-348,449-466;
UniMoE_Audio.py:137-138).

The tokenizer (HF files under `model_path`) and the DAC weights (weights_16khz.pth) are assets that are not available offline; they
are loaded lazily and a clear error is raised when they are missing.  The codec itself runs on the HIP path (unimoe_audio_amd/dac.py).
tests/test_gpu_api.py drives text_to_speech / text_to_music end to end with a stand-in tokenizer and a randomly initialised codec.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, List, NamedTuple, Optional, Sequence, Union

import torch

from .codec_utils import DecoderOutput, generate_output, prepare_audio_prompt, preprocess_codec
from .config import UniMoEAudioConfig
from .model import UniAudioRVQQwen2_5VLMoEForConditionalGeneration
from .prefix_plan import split_point
from .row_params import scaled as _scaled
from .serve import VoicePrompt


class AudioChunk(NamedTuple):
    """One piece of a streamed request: samples [start_sample, start_sample + len(pcm)) of row `row` (float32, CPU, the codec's
    sample rate); `final` on the row's last chunk, which carries the min_duration zero pad of the non-streaming methods."""
    row: int
    start_sample: int
    pcm: torch.Tensor
    final: bool


class _ChunkAssembler:
    """The host side of a streamed read, for _stream_audio and serve(stream=True) alike: what a decoder's push and flush returned becomes
    AudioChunks with one copy to the host; per request (keyed by the chunks' `row`) it tracks the next start sample and, with an
    output_dir, keeps the PCM for the wav that write() saves."""

    def __init__(self, sample_rate: int, output_dir: Optional[str]):
        self.sample_rate, self.output_dir = sample_rate, output_dir
        self.start, self.kept = {}, {}

    def read(self, out: dict, tail: dict, rows):
        """out / tail: {decoder row: samples} of this read's push / flush; rows: [(decoder row, request key, complete)] -> yields
        (decoder row, AudioChunk) for every row with samples or at its end"""
        parts = [(row, key, complete, [t for t in (out.get(row), tail.get(row)) if t is not None]) for row, key, complete in rows]
        flat = [t for *_, ts in parts for t in ts]
        host = torch.cat(flat).float().cpu() if flat else torch.zeros(0)      # one copy to the host per read
        o = 0
        for row, key, complete, ts in parts:
            n = sum(t.numel() for t in ts)
            pcm, o = host[o:o + n], o + n
            if n == 0 and not complete:
                continue
            chunk = AudioChunk(key, self.start.get(key, 0), pcm, complete)
            self.start[key] = chunk.start_sample + n
            if self.output_dir is not None:
                self.kept.setdefault(key, []).append(pcm)
            yield row, chunk

    def write(self, key, name: str):
        """generated_<name>_<key>.wav from the PCM kept for request `key`"""
        from .dac import write_wav_pcm16
        os.makedirs(self.output_dir, exist_ok=True)
        write_wav_pcm16(os.path.join(self.output_dir, f"generated_{name}_{key}.wav"), torch.cat(self.kept.pop(key))[None], self.sample_rate)


# serve(stream=True): do the rows' DAC windows go through the per-row table kernels, one launch per layer (True), or through one
# umoe_dac_*_win launch per layer and row (False)?  Decided by scripts/serve_stream_bench.py (profiles/serve_stream.json).
SERVE_STREAM_RAGGED = True


def _frame_codes(eng, row: int, f0: int, f1: int, t_valid: int) -> torch.Tensor:
    """codes [f1 - f0, C] (int64, CPU) of frames [f0, f1) of `row`, read from the engine's delayed token buffer as generate_output
    reverts them: tokens[row][prefill_step + t + delay_c][c], the pad code at positions >= t_valid (DecodeEngine.finish())"""
    cfg = eng.cfg
    tok = eng.tokens[row]
    d = torch.tensor(list(cfg.codec_delay_pattern), device=tok.device)
    idx = eng.prefill_steps[row] + torch.arange(f0, f1, device=tok.device)[:, None] + d[None]
    g = tok.gather(0, idx.clamp(max=tok.shape[0] - 1)).long()
    return torch.where(idx < t_valid, g, torch.full_like(g, cfg.codec_pad_value)).cpu()


@dataclass
class SpeechRequest:
    """One text_to_speech request of UniMoEAudio.generate_batch: text_to_speech's arguments and defaults, for ONE sentence, plus seed"""
    transcription: str
    prompt_transcription: str
    prompt_wav: Optional[str] = None
    prompt_codec: Any = None
    max_audio_seconds: int = 10
    min_audio_seconds: int = 2
    temperature: float = 1.0
    top_p: float = 1.0
    cfg_filter_top_k: Optional[int] = 45
    save_name: str = "speech"
    cfg_scale: float = 1.0
    eos_prob_mul_factor: float = 1.0
    do_sample: bool = True
    seed: int = 0
    voice: Optional[VoicePrompt] = None      # UniMoEAudio.voice(...): stands for prompt_wav / prompt_codec, and serve() reuses its prefilled prefix


@dataclass
class MusicRequest:
    """One text_to_music request of UniMoEAudio.generate_batch: text_to_music's arguments and defaults, for ONE caption, plus seed"""
    caption: str
    max_audio_seconds: int = 20
    min_audio_seconds: int = 8
    temperature: float = 1.0
    top_p: float = 1.0
    cfg_filter_top_k: Optional[int] = 45
    save_name: str = "music"
    cfg_scale: float = 10.0
    eos_prob_mul_factor: float = 0.6
    do_sample: bool = True
    seed: int = 0


SYSTEM_MESSAGE = "<|im_start|>system\nYou are a helpful assistant.<|im_end|>\n"
INPUT_FORMAT = "<|im_start|>user\n{}<|im_end|>\n<|im_start|>assistant\n"
AUDIO_START = "<|AUDIO_START|>"


class UniMoEAudio:
    def __init__(self, model_path: Optional[str], device_id: int = 0, config: Optional[UniMoEAudioConfig] = None,
                 model: Optional[UniAudioRVQQwen2_5VLMoEForConditionalGeneration] = None, expert_weights: str = "bf16",
                 dac_conv: str = "direct"):
        """expert_weights "fp8": weight-only fp8 (e4m3, one power-of-two scale per row) of the routed and shared experts
        (model.quantize_experts_): decode streams half the expert bytes, at every batch size from 1 to 32 requests; the whole model then
        computes with the dequantized weights.  "fp8-only": the same, and the bf16 expert parameters are released -- each expert as soon
        as it is loaded and quantized -- so the device holds the fp8 copy of every expert and nothing else (inference only: prefill runs
        on the fp8 copies too, the module forward / training / saving raise).  "w12-only": the bf16 expert parameters are released
        in favour of the LOSSLESS 12-bit copies that bf16 engines decode from anyway; prefill runs on them too and no bit of any result
        changes (inference only, like fp8-only).
        dac_conv "mfma": the codec this object builds runs its convolutions on the f32 MFMA kernels (dac.Dac(conv_form=...)):
        exact fp32 arithmetic in another summation order, so waveforms differ from "direct" in the last bits.  Everything that encodes or
        decodes audio (text_to_*, their _stream twins, serve, voice) follows the codec; one assigned through `dac` keeps its own form."""
        if dac_conv not in ("direct", "mfma"):
            raise ValueError(f"dac_conv must be 'direct' or 'mfma' (got {dac_conv!r})")
        self.dac_conv = dac_conv
        if expert_weights not in ("bf16", "fp8", "fp8-only", "w12-only"):
            raise ValueError(f"expert_weights must be 'bf16', 'fp8', 'fp8-only' or 'w12-only' (got {expert_weights!r})")
        if not torch.cuda.is_available():
            raise RuntimeError("UniMoEAudio needs a ROCm device: the accelerated path has no CPU fallback")
        torch.cuda.set_device(device_id)
        self.device = torch.device(f"cuda:{device_id}")
        self.TORCH_DTYPE = torch.bfloat16
        self.model_path = model_path
        if model is not None:
            self.model = model
        else:
            cfg = config
            if cfg is None:
                if not model_path or not os.path.exists(os.path.join(model_path, "config.json")):
                    raise FileNotFoundError("model_path must contain the reference config.json (and the safetensors shards)")
                cfg = UniMoEAudioConfig.from_json(os.path.join(model_path, "config.json"))
            if expert_weights in ("fp8-only", "w12-only"):
                from . import checkpoint
                # built on the device, each expert quantized and released as its tensors arrive: the bf16 experts are never all resident
                self.model = checkpoint.from_pretrained(UniAudioRVQQwen2_5VLMoEForConditionalGeneration, model_path or "", device=self.device,
                                                        config=cfg, expert_weights=expert_weights)
            else:
                self.model = UniAudioRVQQwen2_5VLMoEForConditionalGeneration(cfg)
                self._load_weights(model_path)
                self.model = self.model.to(self.device, torch.bfloat16).eval()
        if expert_weights == "fp8":
            self.model.quantize_experts_("fp8")
        elif expert_weights == "fp8-only":
            self.model.quantize_experts_("fp8", keep_bf16=False)      # (a model handed in; a loaded one is already there: idempotent)
        elif expert_weights == "w12-only":
            self.model.quantize_experts_("w12", keep_bf16=False)
        self._tokenizer = None
        self._dac = None

    # ---- third-party assets ---------------------------------------------------------------------------------------
    def _load_weights(self, model_path):
        from . import checkpoint
        checkpoint.load_checkpoint(self.model, model_path or "")      # HF shards (+ index), reference key spelling, streamed

    @property
    def tokenizer(self):
        if self._tokenizer is None:
            from transformers import AutoTokenizer
            self._tokenizer = AutoTokenizer.from_pretrained(self.model_path, padding_side="left", use_fast=False)
        return self._tokenizer

    @property
    def dac(self):
        """The DAC codec on the HIP path (unimoe_audio_amd/dac.py; reference utils/UniMoE_Audio_utils.py:56-134).  Weights are looked
        for like the reference does (DAC_WEIGHTS, <model_path>/dac_model/weights_16khz.pth, ...); FileNotFoundError when absent."""
        if self._dac is None:
            from .dac import Dac
            cand = None
            if self.model_path:
                for p in (os.path.join(self.model_path, "dac_model", "weights_16khz.pth"), os.path.join(self.model_path, "weights_16khz.pth")):
                    if os.path.isfile(p):
                        cand = p
                        break
            self._dac = Dac(cand, device=self.device, conv_form=self.dac_conv)
        return self._dac

    @dac.setter
    def dac(self, codec):
        self._dac = codec

    # ---- the accelerated part: tokens in, codes out -----------------------------------------------------------------
    @torch.no_grad()
    def generate_codes(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, codec_input_ids: Optional[torch.Tensor] = None,
                       max_audio_seconds: int = 10, min_audio_seconds: int = 2, cfg_scale: float = 3.0, temperature: float = 1.2,
                       top_p: float = 0.95, cfg_filter_top_k: int = 45, eos_prob_mul_factor: float = 0.8, do_sample: bool = True,
                       seed: int = 0):
        """input_ids [2B, T] (negative prompt, positive prompt per sample), returns the list of [len_i, 12] code tensors
        exactly as the reference's `generate_output` does (delay pattern reverted).
        max_audio_seconds, min_audio_seconds, the sampling settings and seed may each be a sequence of B values, one per sample
        (model.generate): the samples then decode in one batch, each with its own settings and length."""
        cfg = self.model.config
        B = input_ids.shape[0] // 2
        prefill, steps = prepare_audio_prompt(cfg, [None] * B)
        dec = DecoderOutput(prefill, steps, self.device)
        codes, lengths = self.model.generate(input_ids, attention_mask, dec, max_tokens=_scaled(max_audio_seconds, 50),
                                             min_tokens=_scaled(min_audio_seconds, 50), codec_input_ids=codec_input_ids,
                                             cfg_scale=cfg_scale, temperature=temperature, top_p=top_p,
                                             cfg_filter_top_k=cfg_filter_top_k, eos_prob_mul_factor=eos_prob_mul_factor,
                                             do_sample=do_sample, seed=seed)
        if codes is None:
            return []
        return generate_output(cfg, codes, lengths)

    def _stream_updates(self, input_ids, attention_mask, codec_input_ids, max_audio_seconds, min_audio_seconds, chunk_frames, **gen):
        B = input_ids.shape[0] // 2
        prefill, steps = prepare_audio_prompt(self.model.config, [None] * B)
        dec = DecoderOutput(prefill, steps, self.device)
        return self.model.generate_stream(input_ids, attention_mask, dec, max_tokens=_scaled(max_audio_seconds, 50),
                                          min_tokens=_scaled(min_audio_seconds, 50),
                                          codec_input_ids=codec_input_ids, chunk_frames=chunk_frames, **gen)

    @torch.no_grad()
    def generate_codes_stream(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, codec_input_ids: Optional[torch.Tensor] = None,
                              max_audio_seconds: int = 10, min_audio_seconds: int = 2, cfg_scale: float = 3.0, temperature: float = 1.2,
                              top_p: float = 0.95, cfg_filter_top_k: int = 45, eos_prob_mul_factor: float = 0.8, do_sample: bool = True,
                              seed: int = 0, chunk_frames: int = 25):
        """generate_codes() as a stream: yields (row, codes [n, 12]) as the decode loop makes frames final, every `chunk_frames`
        steps.  Concatenated per row, the chunks are generate_codes()'s codes at the same seed.  The settings take sequences as
        generate_codes()'s do; a row with a shorter max_audio_seconds is complete while the longer rows still decode."""
        upds = self._stream_updates(input_ids, attention_mask, codec_input_ids, max_audio_seconds, min_audio_seconds, chunk_frames,
                                    cfg_scale=cfg_scale, temperature=temperature, top_p=top_p, cfg_filter_top_k=cfg_filter_top_k,
                                    eos_prob_mul_factor=eos_prob_mul_factor, do_sample=do_sample, seed=seed)
        for upd in upds:
            for row, f0, f1, _ in upd.rows:
                if f1 > f0:
                    yield row, _frame_codes(self.model._engine, row, f0, f1, upd.dec_step + 1)

    @torch.no_grad()
    def _stream_audio(self, input_ids, attention_mask, codec_input_ids, max_audio_seconds, min_audio_seconds, chunk_frames, output_dir, stem,
                      **gen):
        """The streamed twin of generate_codes + _finish: every state read, the frames that became final go through
        umoe_rvq_from_delayed and the streaming DAC decoder, queued on the decode stream between two replays (never on a side
        stream: see DecodeEngine.run_stream).  A row's last chunk carries _finish's min_duration=1 zero pad.
        stem: one save_name, or one per row (generate_batch)."""
        from .dac import DacStreamDecoder, DelayedTokenSource
        B = input_ids.shape[0] // 2
        dm = self.dac.model
        decoder = source = None
        chunks = _ChunkAssembler(dm.sample_rate, output_dir)
        for upd in self._stream_updates(input_ids, attention_mask, codec_input_ids, max_audio_seconds, min_audio_seconds, chunk_frames, **gen):
            if decoder is None:
                source = DelayedTokenSource(self.model._engine, dm)
                decoder = DacStreamDecoder(dm, B, source)
            source.t_valid = upd.dec_step + 1
            n_new = [0] * B
            for row, f0, f1, _ in upd.rows:
                n_new[row] = f1 - f0
            out = decoder.push(n_new)
            ends = [row for row, _, _, complete in upd.rows if complete]
            tail = decoder.flush(ends, min_duration=1) if ends else {}
            for _, chunk in chunks.read(out, tail, [(row, row, complete) for row, _, _, complete in upd.rows]):
                yield chunk
        if output_dir is not None:                         # (the wavs at the end of the stream, as the non-streaming methods write them)
            for i in range(B):
                chunks.write(i, stem if isinstance(stem, str) else stem[i])

    # ---- reference task methods (both spellings) -----------------------------------------------------------------------
    def _texts(self, obj: Union[str, List[str]]) -> List[str]:
        if isinstance(obj, str):
            obj = [obj]
        obj = [c for c in obj if c.strip()]
        if not obj:
            raise ValueError("Please enter valid target texts.")        # UniMoE_Audio.py:94-103
        return obj

    def _finish(self, audios, output_dir, stem):
        os.makedirs(output_dir, exist_ok=True)
        paths = []
        for i, a in enumerate(audios):
            path = os.path.join(output_dir, f"generated_{stem if isinstance(stem, str) else stem[i]}_{i}.wav")
            self.dac.decode(a.transpose(0, 1).unsqueeze(0), save_path=path, min_duration=1)
            paths.append(path)
        return paths

    def text_to_music(self, caption: Union[str, List[str]], output_dir: str = "./", max_audio_seconds: int = 20,
                      min_audio_seconds: int = 8, temperature: float = 1.0, top_p: float = 1.0, cfg_filter_top_k: int = 45,
                      save_name: str = "music", cfg_scale: float = 10.0, eos_prob_mul_factor: float = 0.6, do_sample: bool = True,
                      seed: int = 0, **_) -> List[str]:
        enc = self._music_prompt(caption)
        audios = self.generate_codes(enc.input_ids, enc.attention_mask, None, max_audio_seconds, min_audio_seconds, cfg_scale,
                                     temperature, top_p, cfg_filter_top_k, eos_prob_mul_factor, do_sample, seed)
        return self._finish(audios, output_dir, save_name)

    def _music_prompt(self, caption):
        caption = self._texts(caption)
        neg = SYSTEM_MESSAGE + INPUT_FORMAT.format("<|MUSIC_START|>Low quality.<|MUSIC_END|>") + AUDIO_START
        texts = []
        for c in caption:
            texts += [neg, SYSTEM_MESSAGE + INPUT_FORMAT.format("<|MUSIC_START|>" + c + "<|MUSIC_END|>") + AUDIO_START]
        return self.tokenizer(texts, add_special_tokens=False, return_tensors="pt", padding=True)

    def text_to_music_stream(self, caption: Union[str, List[str]], output_dir: Optional[str] = None, max_audio_seconds: int = 20,
                             min_audio_seconds: int = 8, temperature: float = 1.0, top_p: float = 1.0, cfg_filter_top_k: int = 45,
                             save_name: str = "music", cfg_scale: float = 10.0, eos_prob_mul_factor: float = 0.6, do_sample: bool = True,
                             chunk_frames: int = 25, seed: int = 0, **_):
        """text_to_music() as a stream of AudioChunks (see _stream_audio); output_dir: also write text_to_music()'s wav files at the end"""
        enc = self._music_prompt(caption)
        return self._stream_audio(enc.input_ids, enc.attention_mask, None, max_audio_seconds, min_audio_seconds, chunk_frames, output_dir,
                                  save_name, cfg_scale=cfg_scale, temperature=temperature, top_p=top_p, cfg_filter_top_k=cfg_filter_top_k,
                                  eos_prob_mul_factor=eos_prob_mul_factor, do_sample=do_sample, seed=seed)

    def text_to_speech(self, transcription: Union[str, List[str], None] = None, prompt_transcription: Optional[str] = None,
                       prompt_wav: Optional[str] = None, output_dir: str = "./", max_audio_seconds: int = 10,
                       min_audio_seconds: int = 2, temperature: float = 1.0, top_p: float = 1.0, cfg_filter_top_k: int = 45,
                       caption=None, prompt_text=None, prompt_codec=None, save_name: str = "speech", cfg_scale: float = 1.0,
                       eos_prob_mul_factor: float = 1.0, do_sample: bool = True, seed: int = 0, voice: Optional[VoicePrompt] = None,
                       **_) -> List[str]:
        """voice: a VoicePrompt (UniMoEAudio.voice) in place of prompt_wav / prompt_codec: its reference audio is already encoded"""
        enc, codec = self._speech_prompt(transcription, prompt_transcription, prompt_wav, caption, prompt_text, prompt_codec, voice)
        audios = self.generate_codes(enc.input_ids, enc.attention_mask, codec, max_audio_seconds, min_audio_seconds, cfg_scale,
                                     temperature, top_p, cfg_filter_top_k, eos_prob_mul_factor, do_sample, seed)
        return self._finish(audios, output_dir, save_name)

    def _speech_prompt(self, transcription, prompt_transcription, prompt_wav, caption, prompt_text, prompt_codec, voice=None):
        texts_in = self._texts(transcription if transcription is not None else caption)
        ptxt = prompt_transcription if prompt_transcription is not None else prompt_text
        if voice is not None:
            pc = voice.pc
            ptxt = voice.prompt_transcription if ptxt is None else ptxt
        else:
            if prompt_codec is None:
                if prompt_wav is None:
                    raise ValueError("Please provide a reference audio file.")
                prompt_codec = self.dac.encode(prompt_wav)
            pc = preprocess_codec(self.model.config, prompt_codec)
        texts = []
        for t in texts_in:
            texts += self._speech_texts(ptxt, pc.shape[0], t)
        enc = self.tokenizer(texts, add_special_tokens=False, return_tensors="pt", padding=True)
        codec = pc.unsqueeze(0).expand(len(texts), -1, -1).reshape(-1, pc.shape[1])
        return enc, codec

    @staticmethod
    def _voice_prefix_text(ptxt: str, n_placeholders: int) -> str:
        """the text every prompt of one voice begins with, negative and positive row alike: up to and including <|SPEECH_START|>"""
        return (SYSTEM_MESSAGE + INPUT_FORMAT.split("{}")[0] + "<|SPEECH_PROMPT_START|>" + ptxt + "<|SPEECH_PROMPT_END|>" + "<|VOICE_PROMPT_START|>" +
                "<|AUDIO_PLACEHOLDER|>" * n_placeholders + "<|VOICE_PROMPT_END|>" + "<|SPEECH_START|>")

    def _speech_texts(self, ptxt: str, n_placeholders: int, sentence: str) -> List[str]:
        """the (negative, positive) prompt pair of one sentence"""
        head, tail = self._voice_prefix_text(ptxt, n_placeholders), "<|SPEECH_END|>" + INPUT_FORMAT.split("{}")[1] + AUDIO_START
        return [head + tail, head + sentence + tail]

    @torch.no_grad()
    def voice(self, prompt_transcription: str, prompt_wav: Optional[str] = None, prompt_codec=None) -> VoicePrompt:
        """A voice to speak many sentences in: the reference audio is encoded once, its prompt prefix (system message, prompt
        transcription, the audio placeholders, up to and including <|SPEECH_START|>) tokenised and embedded once, and serve() prefills
        that prefix once per engine and installs its K / V into every request of the voice (SpeechRequest.voice)."""
        if prompt_codec is None:
            if prompt_wav is None:
                raise ValueError("Please provide a reference audio file.")
            prompt_codec = self.dac.encode(prompt_wav)
        pc = preprocess_codec(self.model.config, prompt_codec)
        enc = self.tokenizer([self._voice_prefix_text(prompt_transcription, pc.shape[0])], add_special_tokens=False, return_tensors="pt", padding=True)
        ids = enc.input_ids[0][enc.attention_mask[0].bool()]
        x = self.model.calculate_input_embedding(ids[None].to(self.device), pc.to(self.device))[0].contiguous()
        return VoicePrompt(prompt_transcription, prompt_codec, pc, ids.tolist(), x)

    def text_to_speech_stream(self, transcription: Union[str, List[str], None] = None, prompt_transcription: Optional[str] = None,
                              prompt_wav: Optional[str] = None, output_dir: Optional[str] = None, max_audio_seconds: int = 10,
                              min_audio_seconds: int = 2, temperature: float = 1.0, top_p: float = 1.0, cfg_filter_top_k: int = 45,
                              caption=None, prompt_text=None, prompt_codec=None, save_name: str = "speech", cfg_scale: float = 1.0,
                              eos_prob_mul_factor: float = 1.0, do_sample: bool = True, chunk_frames: int = 25, seed: int = 0,
                              voice: Optional[VoicePrompt] = None, **_):
        """text_to_speech() as a stream of AudioChunks (see _stream_audio); output_dir: also write text_to_speech()'s wav files at the end"""
        enc, codec = self._speech_prompt(transcription, prompt_transcription, prompt_wav, caption, prompt_text, prompt_codec, voice)
        return self._stream_audio(enc.input_ids, enc.attention_mask, codec, max_audio_seconds, min_audio_seconds, chunk_frames, output_dir,
                                  save_name, cfg_scale=cfg_scale, temperature=temperature, top_p=top_p, cfg_filter_top_k=cfg_filter_top_k,
                                  eos_prob_mul_factor=eos_prob_mul_factor, do_sample=do_sample, seed=seed)

    def generate_batch(self, requests: Sequence[Union[SpeechRequest, MusicRequest]], output_dir: Optional[str] = "./", stream: bool = False,
                       chunk_frames: int = 25):
        """Speech and music requests with their OWN settings, lengths and seeds in ONE decode batch: a decode step streams the same
        weights whatever it carries, so a mixed batch costs one generation instead of one per kind of request.
        Each request's prompt pair is built as text_to_speech / text_to_music build it, the pairs are left-padded to one length, and
        one generation runs with the per-request settings table (model.generate).  Returns one wav path per request,
        `generated_<save_name>_<i>.wav` with i the request's position; stream=True returns the generator of AudioChunks instead
        (row = position; output_dir, when not None, also gets the wav files at the end).
        Voice prompts: every SpeechRequest carries its own (prompt_wav or prompt_codec, as text_to_speech requires); music requests
        have none.  The two mix freely: the prompt codes fill the <|AUDIO_PLACEHOLDER|> positions of the batch in row order
        (calculate_input_embedding), and a music prompt has no such position.  video_text_to_music requests are not batched here."""
        if not requests:
            raise ValueError("generate_batch: no requests")
        encs, codecs = [], []
        for r in requests:
            if isinstance(r, SpeechRequest):
                enc, codec = self._speech_prompt(r.transcription, r.prompt_transcription, r.prompt_wav, None, None, r.prompt_codec, r.voice)
                codecs.append(codec)
            elif isinstance(r, MusicRequest):
                enc = self._music_prompt(r.caption)
            else:
                raise TypeError(f"generate_batch: a SpeechRequest or a MusicRequest, not {type(r).__name__}")
            if enc.input_ids.shape[0] != 2:
                raise ValueError("generate_batch: one text per request")
            encs.append(enc)
        T = max(e.input_ids.shape[1] for e in encs)
        pad_id = getattr(self.tokenizer, "pad_token_id", None) or 0
        ids = torch.full((2 * len(encs), T), pad_id, dtype=encs[0].input_ids.dtype)
        mask = torch.zeros((2 * len(encs), T), dtype=encs[0].attention_mask.dtype)
        for i, e in enumerate(encs):                                  # left padding, like the tokenizer's own (mod.py:104)
            ids[2 * i:2 * i + 2, T - e.input_ids.shape[1]:] = e.input_ids
            mask[2 * i:2 * i + 2, T - e.input_ids.shape[1]:] = e.attention_mask
        codec = torch.cat(codecs) if codecs else None
        col = lambda f: [getattr(r, f) for r in requests]            # noqa: E731
        gen = dict(cfg_scale=col("cfg_scale"), temperature=col("temperature"), top_p=col("top_p"), cfg_filter_top_k=col("cfg_filter_top_k"),
                   eos_prob_mul_factor=col("eos_prob_mul_factor"), do_sample=col("do_sample"), seed=col("seed"))
        if stream:
            return self._stream_audio(ids, mask, codec, col("max_audio_seconds"), col("min_audio_seconds"), chunk_frames, output_dir,
                                      col("save_name"), **gen)
        if output_dir is None:
            raise ValueError("generate_batch: output_dir is needed unless stream=True")
        audios = self.generate_codes(ids, mask, codec, col("max_audio_seconds"), col("min_audio_seconds"), **gen)
        return self._finish(audios, output_dir, col("save_name"))

    @torch.no_grad()
    def serve(self, requests, slots: int = 8, output_dir: Optional[str] = "./", poll_every: int = 16, max_prompt_tokens: int = 512,
              max_audio_seconds: int = 20, use_graph: bool = True, expert_weights: Optional[str] = None, w12_wide: Optional[bool] = None,
              prefix_cache: bool = False, prefix_cache_voices: int = 8, stream: bool = False, stream_ragged: Optional[bool] = None):
        """Continuous batching: a generator that takes SpeechRequest / MusicRequest objects from any iterable (read lazily) and yields
        (index, wav path) as each request ends -- index = the request's position in `requests`, the file is
        `generated_<save_name>_<index>.wav`; output_dir=None yields (index, codes [len, C]) instead.  `slots` rows (1..32) decode together,
        above 8 in the wide decode step (every weight streamed once for all rows; with fp8 expert weights its gate/up and down launches
        stream the fp8 copies); a request is admitted into a row as soon as one is free (first in, first out, checked every `poll_every` steps), while the other
        rows keep decoding (DecodeEngine.admit, unimoe_audio_amd/serve.py).  Each request's prompt pair is built as generate_batch builds it
        and keeps its own length.  The engine is sized once: max_prompt_tokens per prompt, max_audio_seconds per request; a request beyond
        either is refused when its turn comes.  `w12_wide`: above 8 slots, bf16 expert weights stream as their lossless 12-bit copies in the wide
        step (model.engine).  Not for expert-parallel engines or video prompts.
        stream=True: the generator yields AudioChunk(row=<request index>, start_sample, pcm, final) instead, every `poll_every` steps for
        every live request whose frames became final: chunks of different requests interleave, the chunks of one request are
        contiguous, its `final` chunk carries the min_duration=1 pad, and concatenated they are the samples of the wav the non-streaming
        path writes.  With output_dir set that wav is written when the final chunk is produced (output_dir=None is allowed: the chunks
        are the result).  Every row decodes its audio on a timeline of its own (dac.DacRowStreamDecoder), queued on the decode stream
        between two steps.  stream_ragged: True = one launch per DAC layer for all rows, False = one per layer and row with news;
        None = SERVE_STREAM_RAGGED, the measured default.
        `prefix_cache`: speech requests with equal (prompt_transcription, prompt_wav or id(prompt_codec)) share a VoicePrompt: the voice's
        prompt prefix is prefilled once per engine, and every admission installs its K / V and prefills only the sentence behind it
        (DESIGN 4n); at most `prefix_cache_voices` voices are kept, least recently used first out.  A request that carries its own
        `voice` takes that path whatever the switch says.  self.served_prefix = {index: (hit, P)} tells per request whether the
        prefix store was there already and how many tokens it covered ((False, 0): admitted in one piece)."""
        from .serve import MAX_SLOTS_WIDE, Scheduler, VoiceLRU
        if not 1 <= slots <= MAX_SLOTS_WIDE:
            raise ValueError(f"serve: slots must be 1..{MAX_SLOTS_WIDE} (got {slots})")
        cfg = self.model.config
        eng = self.model.engine(slots, int(max_prompt_tokens), 50 * int(max_audio_seconds), expert_weights=expert_weights, w12_wide=w12_wide)
        eng.start_serving(int(max_prompt_tokens))
        app = self
        voices = VoiceLRU(prefix_cache_voices) if prefix_cache else None
        prefix_log = []                                    # (hit, P) per admission, in admission order
        emitted = {}                                       # stream=True: row -> frames of its request handed out so far

        class Rows:
            """the engine as unimoe_audio_amd.serve.Scheduler drives it"""
            held = {}

            def admit(self, row, r):
                voice = None
                if isinstance(r, SpeechRequest):
                    voice = r.voice
                    if voice is None and voices is not None:
                        key = (r.prompt_transcription, r.prompt_wav if r.prompt_wav is not None else id(r.prompt_codec))
                        voice = voices.get(key, lambda: app.voice(r.prompt_transcription, r.prompt_wav, r.prompt_codec))
                    enc, codec = app._speech_prompt(r.transcription, r.prompt_transcription, r.prompt_wav, None, None, r.prompt_codec, voice)
                elif isinstance(r, MusicRequest):
                    enc, codec = app._music_prompt(r.caption), None
                else:
                    raise TypeError(f"serve: a SpeechRequest or a MusicRequest, not {type(r).__name__}")
                if enc.input_ids.shape[0] != 2:
                    raise ValueError("serve: one text per request")
                if r.max_audio_seconds > max_audio_seconds:
                    raise ValueError(f"serve: a request of {r.max_audio_seconds} s on an engine sized for {max_audio_seconds} s (max_audio_seconds)")
                prefill, steps = prepare_audio_prompt(cfg, [None])
                settings = dict(max_tokens=50 * r.max_audio_seconds, min_tokens=50 * r.min_audio_seconds, cfg_scale=r.cfg_scale,
                                temperature=r.temperature, top_p=r.top_p, top_k=r.cfg_filter_top_k, eos_mul=r.eos_prob_mul_factor,
                                do_sample=r.do_sample, seed=r.seed)
                P = app._split_point(enc, voice) if voice is not None else 0
                if P >= 1:
                    # a miss builds the store through this (free) row and then admits exactly as a hit does
                    store, hit = voice.store_for(eng, P, lambda n: eng.build_prefix(row, voice.x[:n].contiguous()))
                    eng.admit(row, app._suffix_embedding(enc, voice, P), enc.attention_mask, prefill[0], steps[0], prefix=store, prefix_len=P, **settings)
                    prefix_log.append((hit, P))
                else:
                    x = app.model.calculate_input_embedding(enc.input_ids.to(app.device), None if codec is None else codec.to(app.device))
                    eng.admit(row, x.reshape(-1, x.shape[-1]).contiguous(), enc.attention_mask, prefill[0], steps[0], **settings)
                    prefix_log.append((False, 0))
                self.held[row] = r
                emitted[row] = 0

            def steps(self, n):
                for _ in range(n):
                    eng.step(use_graph)

            def poll(self):
                if not stream:
                    return eng.poll()
                state, self.clock = eng.poll_clock()       # the clocks of the same read: what serve.final_frames needs
                return state

            def row_done(self, state, row):
                return eng.row_done(state, row)

            def take(self, row):
                codes, length = eng.take(row)
                return self.held.pop(row), codes, length

        sched = Scheduler(Rows(), slots, poll_every, max_slots=MAX_SLOTS_WIDE)
        self.served_rows = {}                              # request index -> the row it decoded in (of the last / the running serve())
        self.served_prefix = {}                            # request index -> (prefix store hit, prefix tokens P)
        if stream:
            ragged = SERVE_STREAM_RAGGED if stream_ragged is None else bool(stream_ragged)
            yield from self._serve_stream(sched, eng, requests, emitted, prefix_log, output_dir, ragged)
            return
        for index, (r, codes, length) in sched.run(requests):
            self.served_rows.update({i: row for i, row, _ in sched.admitted})
            self.served_prefix.update({i: hp for (i, _, _), hp in zip(sched.admitted, prefix_log)})
            audio = generate_output(cfg, codes[None], torch.tensor([length], device=codes.device))[0]
            if output_dir is None:
                yield index, audio
                continue
            os.makedirs(output_dir, exist_ok=True)
            path = os.path.join(output_dir, f"generated_{r.save_name}_{index}.wav")
            self.dac.decode(audio.transpose(0, 1).unsqueeze(0), save_path=path, min_duration=1)
            yield index, path

    def _serve_stream(self, sched, eng, requests, emitted, prefix_log, output_dir, ragged):
        """serve(stream=True): at every poll, before an ended row is taken and the next request admitted into it (Scheduler.run's
        hook), the frames that became final on each row's own clock (serve.final_frames) go through umoe_rvq_from_delayed_rows and the
        per-row DAC decoder; rows that ended are flushed (min_duration=1, as _finish pads) and reset for their next request."""
        from .dac import DacRowStreamDecoder, DelayedRowsSource
        from .serve import final_frames
        dm = self.dac.model
        md = max(self.model.config.codec_delay_pattern)
        source = DelayedRowsSource(eng, dm)                # (refuses a DAC with fewer codebooks than codec channels)
        decoder = DacRowStreamDecoder(dm, sched.slots, source, max_frames=sched.poll_every, ragged=ragged)
        self.serve_decoder = decoder
        assembler = _ChunkAssembler(dm.sample_rate, output_dir)

        def hook(state):
            frames = final_frames(state.tolist(), sched.engine.clock.tolist(), eng.prefill_steps, md, {row: emitted[row] for row in sched.live})
            n_new = [0] * sched.slots
            for fr in frames:
                source.t_valid[fr.row], n_new[fr.row], emitted[fr.row] = fr.t_valid, fr.f1 - fr.f0, fr.f1
            out = decoder.push(n_new)
            ends = [fr.row for fr in frames if fr.complete]
            tail = decoder.flush(ends, min_duration=1) if ends else {}
            chunks = []
            for row, chunk in assembler.read(out, tail, [(fr.row, sched.live[fr.row], fr.complete) for fr in frames]):
                chunks.append(chunk)
                if chunk.final:                            # the row's request has ended: its wav now, the row ready for the next one
                    decoder.reset(row)
                    if output_dir is not None:
                        assembler.write(chunk.row, sched.engine.held[row].save_name)
            return chunks

        for item in sched.run(requests, hook):
            self.served_rows.update({i: row for i, row, _ in sched.admitted})
            self.served_prefix.update({i: hp for (i, _, _), hp in zip(sched.admitted, prefix_log)})
            if isinstance(item, AudioChunk):
                yield item
            elif item[1][2] != emitted[self.served_rows[item[0]]]:      # (index, (request, codes, length)): the row as take() has it
                raise AssertionError(f"serve: request {item[0]} streamed {emitted[self.served_rows[item[0]]]} frames, take() has {item[1][2]}")

    def _split_point(self, enc, voice: VoicePrompt) -> int:
        """P of a request in `voice`: the longest common prefix of the pair's id rows and the voice's prefix ids, clamped to T - 2; 0 when
        an audio placeholder would stay behind it (the columns behind the prefix are embedded as text)"""
        T = int(enc.input_ids.shape[1])
        rows = [enc.input_ids[r][enc.attention_mask[r].bool()].tolist() for r in range(2)]
        P = split_point(rows[0], rows[1], voice.ids, T)
        ph = self.model.codec_placeholder_value
        if P < 1 or any(ph in row[P:] for row in rows):
            return 0
        return P

    def _suffix_embedding(self, enc, voice: VoicePrompt, P: int) -> torch.Tensor:
        """[2 * (T - P), D]: columns [P, T) of the pair's embeddings.  Behind its pads the shorter row repeats its last prefix tokens
        there: those come from the voice's embeddings, everything else is text."""
        T = int(enc.input_ids.shape[1])
        x = self.model.language_model.embed_tokens.weight[enc.input_ids[:, P:].to(self.device)]
        for r in range(2):
            first = T - int(enc.attention_mask[r].sum())
            t0, t1 = max(P, first), min(T, first + P)      # column t holds the row's token t - first: a prefix token below first + P
            if t1 > t0:
                x[r, t0 - P:t1 - P] = voice.x[t0 - first:t1 - first]
        return x.reshape(-1, x.shape[-1]).contiguous()

    def video_text_to_music(self, video, caption: Union[str, List[str]], output_dir: str = "./", max_audio_seconds: int = 20,
                            min_audio_seconds: int = 8, temperature: float = 1.0, top_p: float = 1.0, cfg_filter_top_k: int = 45,
                            save_name: str = "video_music", cfg_scale: float = 10.0, eos_prob_mul_factor: float = 0.6, do_sample: bool = True,
                            fps: float = 1.0, sampling_fps: float = 1.0, max_frames: int = 8, vision_in_generate: bool = False, **_) -> List[str]:
        """reference UniMoE_Audio.py:203-257 / utils/UniMoE_Audio_mod.py:483-619: a video (here: its frames, a uint8 / float tensor
        [F, H, W, 3] or [F, 3, H, W]; file decoding needs moviepy / qwen_vl_utils, absent offline) + a caption -> music.  The frames are
        resized to multiples of 28 px within the reference's pixel budget (mod.py:49-53: at most 64 * 28 * 28 per frame), cut into the
        processor's patch layout; their tokens sit between <|vision_start|> and <|vision_end|>.
        vision_in_generate: False (default) = the reference's inference path, whose generate() never feeds the pixels to the model (the
        pad tokens keep their text embeddings, positions stay 1-D; see model.generate); True = vision tower + 3-D positions.
        A file path is decoded when a decoder is importable here (torchvision.io / decord / moviepy, in that order)."""
        enc, vis = self._video_prompt(video, caption, sampling_fps, max_frames)
        R = enc.input_ids.shape[0]
        cfg = self.model.config
        prefill, steps = prepare_audio_prompt(cfg, [None] * (R // 2))
        dec = DecoderOutput(prefill, steps, self.device)
        codes, lengths = self.model.generate(enc.input_ids, enc.attention_mask, dec, max_tokens=max_audio_seconds * 50,
                                             min_tokens=min_audio_seconds * 50, **vis,
                                             cfg_scale=cfg_scale, temperature=temperature, top_p=top_p, cfg_filter_top_k=cfg_filter_top_k,
                                             eos_prob_mul_factor=eos_prob_mul_factor, do_sample=do_sample, vision_in_generate=vision_in_generate)
        audios = [] if codes is None else generate_output(cfg, codes, lengths)
        return self._finish(audios, output_dir, save_name)

    def _video_prompt(self, video, caption, sampling_fps, max_frames):
        """(tokenized prompts, the pixel arguments of generate()) of video_text_to_music"""
        from .vision import frames_to_patches
        caption = self._texts(caption)
        if isinstance(video, (str, bytes, os.PathLike)):
            video = _decode_video_file(os.fspath(video), sampling_fps, max_frames)
        frames = video if torch.is_tensor(video) else torch.as_tensor(video)
        if frames.dim() != 4:
            raise ValueError("video: pass the frames as a [F, H, W, 3] or [F, 3, H, W] tensor (file decoding is not available offline)")
        patches, grid = frames_to_patches(frames[:max_frames], max_pixels=64 * 28 * 28)
        n_tok = int(grid.prod()) // 4
        vid = "<|vision_start|>" + "<|video_pad|>" * n_tok + "<|vision_end|>"
        neg = SYSTEM_MESSAGE + INPUT_FORMAT.format(vid + "<|MUSIC_START|>Low quality.<|MUSIC_END|>") + AUDIO_START
        texts = []
        for c in caption:
            texts += [neg, SYSTEM_MESSAGE + INPUT_FORMAT.format(vid + "<|MUSIC_START|>" + c + "<|MUSIC_END|>") + AUDIO_START]
        enc = self.tokenizer(texts, add_special_tokens=False, return_tensors="pt", padding=True)
        R = len(texts)
        return enc, dict(pixel_values_videos=patches.repeat(R, 1), video_grid_thw=grid[None].repeat(R, 1),
                         second_per_grid_ts=torch.full((R,), 2.0 / max(sampling_fps, 1e-6)))

    def video_text_to_music_stream(self, video, caption: Union[str, List[str]], output_dir: Optional[str] = None, max_audio_seconds: int = 20,
                                   min_audio_seconds: int = 8, temperature: float = 1.0, top_p: float = 1.0, cfg_filter_top_k: int = 45,
                                   save_name: str = "video_music", cfg_scale: float = 10.0, eos_prob_mul_factor: float = 0.6,
                                   do_sample: bool = True, fps: float = 1.0, sampling_fps: float = 1.0, max_frames: int = 8,
                                   vision_in_generate: bool = False, chunk_frames: int = 25, **_):
        """video_text_to_music() as a stream of AudioChunks (see _stream_audio); output_dir: also write its wav files at the end"""
        enc, vis = self._video_prompt(video, caption, sampling_fps, max_frames)
        return self._stream_audio(enc.input_ids, enc.attention_mask, None, max_audio_seconds, min_audio_seconds, chunk_frames, output_dir,
                                  save_name, cfg_scale=cfg_scale, temperature=temperature, top_p=top_p, cfg_filter_top_k=cfg_filter_top_k,
                                  eos_prob_mul_factor=eos_prob_mul_factor, do_sample=do_sample, vision_in_generate=vision_in_generate, **vis)


def _decode_video_file(path: str, sampling_fps: float, max_frames: int) -> torch.Tensor:
    """Frames [F, H, W, 3] uint8 of a video file, sampled at `sampling_fps` (reference utils/UniMoE_Audio_mod.py:158-213 uses moviepy +
    qwen_vl_utils).  Tries the decoders that may be importable here; raises a ValueError that says what to pass instead when none is."""
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    errors = []
    try:
        from torchvision.io import read_video          # type: ignore
        frames, _, info = read_video(path, pts_unit="sec", output_format="THWC")
        step = max(int(round(float(info.get("video_fps", 1.0)) / max(sampling_fps, 1e-6))), 1)
        return frames[::step][:max_frames]
    except Exception as e:      # not installed, or no backend for the container
        errors.append(f"torchvision.io: {e!r}")
    try:
        import decord                                   # type: ignore
        vr = decord.VideoReader(path)
        step = max(int(round(vr.get_avg_fps() / max(sampling_fps, 1e-6))), 1)
        idx = list(range(0, len(vr), step))[:max_frames]
        return torch.from_numpy(vr.get_batch(idx).asnumpy())
    except Exception as e:
        errors.append(f"decord: {e!r}")
    try:
        from moviepy.editor import VideoFileClip       # type: ignore
        import numpy as np
        clip = VideoFileClip(path)
        ts = [i / max(sampling_fps, 1e-6) for i in range(max_frames) if i / max(sampling_fps, 1e-6) < clip.duration]
        return torch.from_numpy(np.stack([clip.get_frame(t) for t in ts]))
    except Exception as e:
        errors.append(f"moviepy: {e!r}")
    raise ValueError("video: no video decoder is importable here (" + "; ".join(errors) + "): pass the frames as a [F, H, W, 3] or "
                     "[F, 3, H, W] tensor instead")


def create_unimoe_audio(model_path: str, device_id: int = 0) -> UniMoEAudio:
    return UniMoEAudio(model_path, device_id)
