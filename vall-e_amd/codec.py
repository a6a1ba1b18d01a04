"""EnCodec-24 kHz codec on the GPU.  Decode: codec tokens -> waveform, the step `valle/bin/infer.py:251-253` takes right after
`VALLE.inference` (through `valle/data/tokenizer.py:241-242`).  Encode (`encoder=True`): prompt waveform -> codec tokens, the
step `tokenize_audio` takes before it (`valle/data/tokenizer.py:238-254`), at 6 kbps (8 codebooks), mono, one chunk, no
normalisation.  A prompt at another rate or with several channels goes through `Resampler` first (`convert_audio`'s mix-down
and windowed-sinc resampling, in HIP: pass `sr=`), and `decode(..., sr=)` returns the waveform at a caller's rate.  WAV files
are read and written with the standard library (`load_wav`, `save_wav`, `tokenize_audio`).  The kernels are
csrc/codec_kernels.hpp behind `vx_codec_*` / `vx_resample*` (include/vallex.h); there is no CPU fallback.

    dec = EncodecDecoder(max_frames=2048, encoder=True)
    dec.load_state_dict(encodec_model.state_dict(), strict=False)   # decoder.*, encoder.* and quantizer.* keys are taken
    dec.to("cuda")
    codes = dec.encode(prompt_wav)                                  # (1, 1, L) float32 at 24 kHz -> (1, 8, ceil(L / 320)) int64
    wav = dec.decode(frames.transpose(2, 1))                        # frames (1, T, 8) from VALLE.inference -> (1, 1, 320 T)
    codes = dec.encode(stereo_44k, sr=44100)                        # (2, L) at 44.1 kHz: mixed down and resampled on the GPU first
    [(codes, _)] = tokenize_audio(AudioTokenizer(dec), "prompt.wav")
"""
from __future__ import annotations

import ctypes as C
import math
import wave
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine as _e
from ._handle import Handle, i32_array, normalize_device, owner_resampler, prepare_waveforms, ptr_array, shared, to_native_rate

_WN = "parametrizations.weight.original"
SAMPLE_RATE = 24000  # the model's rate


@dataclass(frozen=True)
class CodecConfig:
    """Geometry of the decoder; the defaults are the 24 kHz model (transformers' `EncodecConfig()`)."""
    hidden: int = 128
    filters: int = 32
    ratios: Tuple[int, int, int, int] = (8, 5, 4, 2)
    kernel: int = 7
    last_kernel: int = 7
    res_kernel: int = 3
    lstm_layers: int = 2
    codebook_size: int = 1024
    n_codebooks: int = 8  # 6 kbps, what the reference's tokenizer sets

    @property
    def width(self) -> int:
        return 16 * self.filters

    @property
    def hop(self) -> int:
        return int(np.prod(self.ratios))


def expected_keys(cfg: CodecConfig, encoder: bool = False) -> "OrderedDict[str, Tuple[int, ...]]":
    """Key -> shape with weight norm removed (the names `vx_codec_set_weight` takes): the decoder and the codebooks, then with
    `encoder` the encoder's (its ratios are the decoder's reversed)."""
    W = cfg.width
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["decoder.layers.0.conv.weight"] = (W, cfg.hidden, cfg.kernel)
    s["decoder.layers.0.conv.bias"] = (W,)
    for l in range(cfg.lstm_layers):
        for n, shp in (("weight_ih", (4 * W, W)), ("weight_hh", (4 * W, W)), ("bias_ih", (4 * W,)), ("bias_hh", (4 * W,))):
            s[f"decoder.layers.1.lstm.{n}_l{l}"] = shp
    c = W
    for i, r in enumerate(cfg.ratios):
        up, res = 3 + 3 * i, 4 + 3 * i
        s[f"decoder.layers.{up}.conv.weight"] = (c, c // 2, 2 * r)
        s[f"decoder.layers.{up}.conv.bias"] = (c // 2,)
        c //= 2
        p = f"decoder.layers.{res}."
        s[p + "block.1.conv.weight"] = (c // 2, c, cfg.res_kernel)
        s[p + "block.1.conv.bias"] = (c // 2,)
        s[p + "block.3.conv.weight"] = (c, c // 2, 1)
        s[p + "block.3.conv.bias"] = (c,)
        s[p + "shortcut.conv.weight"] = (c, c, 1)
        s[p + "shortcut.conv.bias"] = (c,)
    last = 3 + 3 * len(cfg.ratios)
    s[f"decoder.layers.{last}.conv.weight"] = (1, c, cfg.last_kernel)
    s[f"decoder.layers.{last}.conv.bias"] = (1,)
    for q in range(cfg.n_codebooks):
        s[f"quantizer.layers.{q}.codebook.embed"] = (cfg.codebook_size, cfg.hidden)
    if not encoder:
        return s
    c = cfg.filters
    s["encoder.layers.0.conv.weight"] = (c, 1, cfg.kernel)
    s["encoder.layers.0.conv.bias"] = (c,)
    for i, r in enumerate(reversed(cfg.ratios)):
        res, down = 1 + 3 * i, 3 + 3 * i
        p = f"encoder.layers.{res}."
        s[p + "block.1.conv.weight"] = (c // 2, c, cfg.res_kernel)
        s[p + "block.1.conv.bias"] = (c // 2,)
        s[p + "block.3.conv.weight"] = (c, c // 2, 1)
        s[p + "block.3.conv.bias"] = (c,)
        s[p + "shortcut.conv.weight"] = (c, c, 1)
        s[p + "shortcut.conv.bias"] = (c,)
        s[f"encoder.layers.{down}.conv.weight"] = (2 * c, c, 2 * r)
        s[f"encoder.layers.{down}.conv.bias"] = (2 * c,)
        c *= 2
    li = 1 + 3 * len(cfg.ratios)
    for l in range(cfg.lstm_layers):
        for n, shp in (("weight_ih", (4 * W, W)), ("weight_hh", (4 * W, W)), ("bias_ih", (4 * W,)), ("bias_hh", (4 * W,))):
            s[f"encoder.layers.{li}.lstm.{n}_l{l}"] = shp
    s[f"encoder.layers.{li + 2}.conv.weight"] = (cfg.hidden, W, cfg.last_kernel)
    s[f"encoder.layers.{li + 2}.conv.bias"] = (cfg.hidden,)
    return s


def pack_state_dict(cfg: CodecConfig, sd: Dict[str, torch.Tensor], strict: bool = True, encoder: bool = False):
    """Either accepted layout -> (fp32 tensors under the plain names, missing, unexpected).  Weight norm (w = g v / |v|, the norm
    over all dimensions but the first) is folded in fp64 and rounded once.  With strict=False keys outside the decoder and
    the loaded codebooks (the encoder unless `encoder`, EMA statistics, further codebooks) are ignored."""
    want = expected_keys(cfg, encoder)
    out: Dict[str, torch.Tensor] = {}
    used = set()
    for k, shp in want.items():
        if k in sd:
            t = sd[k].detach().to("cpu", torch.float64)
            used.add(k)
        elif k.endswith(".conv.weight") and k[:-len("weight")] + _WN + "1" in sd:
            kg, kv = k[:-len("weight")] + _WN + "0", k[:-len("weight")] + _WN + "1"
            if kg not in sd:
                continue
            g, v = sd[kg].detach().to("cpu", torch.float64), sd[kv].detach().to("cpu", torch.float64)
            if g.numel() != v.shape[0]:
                raise RuntimeError(f"size mismatch for {kg}: {tuple(g.shape)} against {tuple(v.shape)}")
            t = g.reshape(-1, 1, 1) * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
            used.update((kg, kv))
        else:
            continue
        if tuple(t.shape) != tuple(shp):
            raise RuntimeError(f"size mismatch for {k}: {tuple(t.shape)}, expected {tuple(shp)}")
        out[k] = t.to(torch.float32).contiguous()
    missing = [k for k in want if k not in out]
    unexpected = [k for k in sd if k not in used]
    if strict and (missing or unexpected):
        raise RuntimeError(f"Error(s) in loading state_dict for EncodecDecoder: missing {missing}, unexpected {unexpected}")
    return out, missing, unexpected


def resample_length(orig_hz: int, new_hz: int, n_samples: int) -> int:
    """ceil(n L / o) with o, n the rates over their gcd: the samples a resampled waveform of L samples has (host only)."""
    r = int(_e.load_library().vx_resample_length(int(orig_hz), int(new_hz), int(n_samples)))
    if r < 0:
        raise ValueError(f"resample_length({orig_hz}, {new_hz}, {n_samples}): rates and length must be positive")
    return r


class Resampler(Handle):
    """`encodec.utils.convert_audio`'s mono path on the GPU: the channel mean, then `torchaudio.transforms.Resample(orig_hz,
    new_hz)` with its defaults (Hann-windowed sinc, width 6, roll-off 0.99; include/vallex.h states the rule).  One rate pair per
    object, up to `max_batch` utterances of any lengths and channel counts per `resample_batch` call."""
    _PREFIX, _NAME = "vx_resampler", "Resampler"  # the call itself is `vx_resample`

    def __init__(self, orig_hz: int, new_hz: int, max_batch: int = 1):
        self.orig_hz, self.new_hz, self.max_batch = int(orig_hz), int(new_hz), int(max_batch)
        self._init_handle()  # a rate pair the kernel does not serve is refused here

    def _create_call(self, lib, out_handle) -> int:
        return lib.vx_resampler_create(self.orig_hz, self.new_hz, self.max_batch, out_handle)

    def output_length(self, n_samples: int) -> int:
        return resample_length(self.orig_hz, self.new_hz, n_samples)

    @torch.no_grad()
    def resample_batch(self, wavs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """wavs[i]: (L_i,), (C_i, L_i) or (1, C_i, L_i) float32 -> [(1, 1, ceil(n L_i / o)) float32 on the device], every utterance
        bitwise what it is alone."""
        ws = []
        for w in wavs:
            assert w.dtype == torch.float32 and 1 <= w.dim() <= 3, "waveforms are float32 (L,), (C, L) or (1, C, L)"
            if w.dim() == 3:
                assert w.shape[0] == 1, "one utterance per entry"
                w = w[0]
            ws.append(w.detach().reshape(-1, w.shape[-1]))
        self._need_device()
        ws = [w.to(self.device).contiguous() for w in ws]
        outs = [torch.empty((1, 1, self.output_length(w.shape[1])), dtype=torch.float32, device=self.device) for w in ws]
        with torch.cuda.device(self.device):
            self._resample_raw([w.data_ptr() for w in ws], [w.shape[0] for w in ws], [w.shape[1] for w in ws],
                               [o.data_ptr() for o in outs])
        return outs

    def _resample_raw(self, in_ptrs, channels, lengths, out_ptrs):
        """vx_resample on raw pointers (the argument checks run before any device work)."""
        self._invoke(_e.load_library().vx_resample, len(in_ptrs), ptr_array(in_ptrs), i32_array(channels), i32_array(lengths),
                     ptr_array(out_ptrs))

    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        return self.resample_batch([wav])[0]


_SHARED: Dict[tuple, Resampler] = {}


def convert_audio(wav: torch.Tensor, sr: int, target_sr: int = 24000, target_channels: int = 1) -> torch.Tensor:
    """`encodec.utils.convert_audio(wav, sr, target_sr, target_channels)` for the mono target: wav (C, L) float32 on the GPU ->
    (1, L') at `target_sr` on the GPU (at sr == target_sr: the channel mean).  Resamplers are kept per rate pair and device."""
    if target_channels != 1:
        raise NotImplementedError(f"convert_audio: target_channels = {target_channels}; the mono target is served")
    assert wav.dim() == 2, "wav is (C, L)"
    if wav.device.type != "cuda":
        raise RuntimeError("valle_amd.convert_audio runs only on an MI355X: move the waveform to 'cuda' first (no CPU fallback)")
    return shared(_SHARED, wav.device, (int(sr), int(target_sr)), lambda: Resampler(sr, target_sr))(wav)[0]


# ---- WAV files (standard library only) ----------------------------------------------------------------------------------
def load_wav(path: str) -> Tuple[torch.Tensor, int]:
    """PCM WAV of 8 (unsigned), 16, 24 or 32 bits -> (wav (C, L) float32 in [-1, 1), sample rate), as `torchaudio.load` scales
    integer PCM: by 2^-(bits - 1)."""
    with wave.open(path, "rb") as f:
        nch, width, sr, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        raw = f.readframes(n)
    if width == 1:
        a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 2:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        a = (v - ((v & 0x800000) << 1)).astype(np.float32) / 8388608.0
    elif width == 4:
        a = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples; PCM of 8, 16, 24 or 32 bits is read")
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1, nch).T)), sr


def save_wav(path: str, wav: torch.Tensor, sr: int) -> None:
    """wav (L,), (C, L) or (1, C, L) float in [-1, 1) -> 16-bit PCM: round(x 32768) clamped to the int16 range."""
    w = wav.detach().to("cpu", torch.float32)
    w = w.reshape(-1, w.shape[-1])
    q = np.clip(np.rint(w.numpy().astype(np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as f:
        f.setnchannels(q.shape[0])
        f.setsampwidth(2)
        f.setframerate(int(sr))
        f.writeframes(np.ascontiguousarray(q.T).tobytes())


def tokenize_audio(tokenizer: "AudioTokenizer", audio_path: str):
    """The reference's `tokenize_audio` (tokenizer.py:245-254): file -> mono at the tokenizer's rate -> `[(codes (1, n_q, T),
    None)]`, with the conversion on the GPU."""
    wav, sr = load_wav(audio_path)
    return tokenizer.encode(wav.unsqueeze(0).to(tokenizer.device), sr=sr)


class EncodecDecoder:
    """codes -> 24 kHz waveform in HIP and, with `encoder=True`, waveform -> codes on the same handle.  `max_frames` / `max_batch`
    are capacities (frames per utterance, i.e. `max_frames * hop` samples to encode, and utterances per `decode_batch` /
    `encode_batch` call; the workspace is allocated for them on first use)."""

    def __init__(self, config: Optional[CodecConfig] = None, max_frames: int = 2048, max_batch: int = 1, lstm_graph: bool = False,
                 encoder: bool = False):
        self.cfg = config or CodecConfig()
        if len(self.cfg.ratios) != 4:
            raise NotImplementedError("four up-sampling stages")
        self.max_frames, self.max_batch = int(max_frames), int(max_batch)
        self.lstm_graph = bool(lstm_graph)  # LSTM steps replayed as a captured chain instead of plain launches (not faster)
        self.encoder = bool(encoder)
        self.device = torch.device("cpu")
        self._sd: Dict[str, torch.Tensor] = {}
        self._h = None
        self._final = False
        self._resamplers: Dict[Tuple[int, int], Resampler] = {}
        self._fbank = None

    # ---- weights ------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = True):
        """Accepts the local EncodecModel's names (`decoder.layers.N.conv.parametrizations.weight.original0/1`, the LSTM's torch
        names, `quantizer.layers.q.codebook.embed`; with `encoder=True` the `encoder.layers.N...` names too) and the same names
        with weight norm removed (`...conv.weight`)."""
        from .models import _IncompatibleKeys

        packed, missing, unexpected = pack_state_dict(self.cfg, state_dict, strict, self.encoder)
        self._sd.update(packed)
        self._drop()
        return _IncompatibleKeys(missing, unexpected)

    def state_dict(self):
        return OrderedDict((k, self._sd[k]) for k in expected_keys(self.cfg, self.encoder) if k in self._sd)

    def to(self, device):
        self.device = normalize_device(device)
        self._drop()
        for r in self._resamplers.values():
            r.close()
        self._resamplers = {}
        if self._fbank is not None:
            self._fbank.close()
            self._fbank = None
        return self

    def fbank(self):
        """The object's log-mel extractor (`fbank.BigVGANFbank` with the reference's settings), made on first use."""
        if self._fbank is None:
            from .fbank import BigVGANFbank

            self._fbank = BigVGANFbank(max_batch=2).to(self.device)
        return self._fbank

    def resampler(self, orig_hz: int, new_hz: int) -> Resampler:
        """The object's `Resampler` for a rate pair (kept per pair, `max_batch` utterances per call)."""
        return owner_resampler(self, orig_hz, new_hz)

    def cuda(self, index: int = 0):
        return self.to(torch.device("cuda", index))

    def eval(self):
        return self

    def _drop(self):
        if self._h is not None:
            _e.load_library().vx_codec_destroy(self._h)
            self._h = None
            self._final = False

    close = _drop

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass

    def _config_struct(self) -> "_e.VxCodecConfig":
        c, g = _e.VxCodecConfig(), self.cfg
        c.struct_size = C.sizeof(_e.VxCodecConfig)
        c.hidden, c.filters, c.kernel, c.last_kernel, c.res_kernel = g.hidden, g.filters, g.kernel, g.last_kernel, g.res_kernel
        for i, r in enumerate(g.ratios):
            c.ratios[i] = r
        c.n_codebooks, c.codebook_size, c.codebook_dim, c.lstm_layers = g.n_codebooks, g.codebook_size, g.hidden, g.lstm_layers
        c.max_frames, c.max_batch, c.device = self.max_frames, self.max_batch, self.device.index or 0
        c.flags = (_e.VX_CODEC_LSTM_GRAPH if self.lstm_graph else 0) | (_e.VX_CODEC_ENCODER if self.encoder else 0)
        return c

    def handle(self, finalize: bool = True):
        """The C handle, created on first use; finalising it needs the GPU (there is no CPU path)."""
        lib = _e.load_library()
        if finalize and self.device.type != "cuda":
            raise RuntimeError("valle_amd.EncodecDecoder runs only on an MI355X: call .to('cuda') first (no CPU fallback)")
        if self._h is None:
            h = C.c_void_p()
            _e._check(lib.vx_codec_create(C.byref(self._config_struct()), C.byref(h)))
            self._h = h
            for k, t in self._sd.items():
                shp = (C.c_int64 * t.dim())(*t.shape)
                _e._check(lib.vx_codec_set_weight(h, k.encode(), t.data_ptr(), shp, t.dim()))
        if finalize and not self._final:
            try:
                _e._check(lib.vx_codec_finalize(self._h))
            except Exception:
                self._drop()  # a handle whose finalize failed refuses further use: the next call starts from a fresh one
                raise
            self._final = True
        return self._h

    # ---- decode -------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode_batch(self, codes: Sequence[torch.Tensor], sr: Optional[int] = None) -> List[torch.Tensor]:
        """codes[i]: (n_q, T_i) or (1, n_q, T_i) int64, the same n_q for all -> [(1, 1, hop T_i) float32 on the device]; with
        `sr` other than 24000 the waveforms are resampled to it on the GPU."""
        cs = []
        for c in codes:
            if c.dim() == 3:
                assert c.shape[0] == 1, "one utterance per entry"
                c = c[0]
            assert c.dim() == 2 and c.dtype == torch.int64, "codes are (n_q, T) int64"
            cs.append(c.detach().to("cpu").contiguous())
        assert cs and all(c.shape[0] == cs[0].shape[0] for c in cs), "every utterance of a call has the same n_q"
        if self.device.type != "cuda":
            raise RuntimeError("valle_amd.EncodecDecoder runs only on an MI355X: call .to('cuda') first (no CPU fallback)")
        outs = [torch.empty((1, 1, self.cfg.hop * c.shape[1]), dtype=torch.float32, device=self.device) for c in cs]
        self._decode_raw(cs, [o.data_ptr() for o in outs])
        if sr is not None and int(sr) != SAMPLE_RATE:
            outs = self.resampler(SAMPLE_RATE, sr).resample_batch(outs)
        return outs

    def _decode_raw(self, cs, out_ptrs, finalize: bool = True):
        """vx_codec_decode on host code tensors and raw output pointers (the argument checks run before any device work)."""
        n = len(cs)
        lib = _e.load_library()
        h = self.handle(finalize)
        cp, T, op = ptr_array([c.data_ptr() for c in cs]), i32_array([c.shape[1] for c in cs]), ptr_array(out_ptrs)
        stream = _e.current_stream_ptr(self.device) if self.device.type == "cuda" else None
        _e._check(lib.vx_codec_decode(h, n, cp, T, cs[0].shape[0], op, stream))

    def decode(self, codes: torch.Tensor, sr: Optional[int] = None) -> torch.Tensor:
        """(1, n_q, T) or (n_q, T) int64 -> (1, 1, hop T) float32 on the device (at `sr`: resampled from 24 kHz)."""
        return self.decode_batch([codes], sr)[0]


    # ---- encode -------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_batch(self, wavs: Sequence[torch.Tensor], n_q: Optional[int] = None, sr: Optional[int] = None) -> List[torch.Tensor]:
        """wavs[i]: (L_i,), (1, L_i) or (1, 1, L_i) float32 mono at 24 kHz, any L_i >= 1 -> [(1, n_q, ceil(L_i / hop)) int64 on the
        device], all utterances in one ragged launch sequence (each bitwise what it gets alone).  With `sr` given the entries
        are (L_i,), (C_i, L_i) or (1, C_i, L_i) at that rate and are mixed down and resampled on the GPU first, as the
        reference's `convert_audio(wav, sr, 24000, 1)` does (mono input at 24000 goes to the encoder as it is)."""
        if not self.encoder:
            raise RuntimeError("this EncodecDecoder was built without encoder=True")
        if self.device.type != "cuda":
            raise RuntimeError("valle_amd.EncodecDecoder runs only on an MI355X: call .to('cuda') first (no CPU fallback)")
        n_q = self.cfg.n_codebooks if n_q is None else int(n_q)
        ws = prepare_waveforms(self, wavs, sr, SAMPLE_RATE, strict=False)
        outs = [torch.empty((1, n_q, -(-w.numel() // self.cfg.hop)), dtype=torch.int64, device=self.device) for w in ws]
        self._encode_raw([w.data_ptr() for w in ws], [w.numel() for w in ws], n_q, [o.data_ptr() for o in outs])
        return outs

    def _encode_raw(self, wav_ptrs, lengths, n_q, out_ptrs, finalize: bool = True):
        """vx_codec_encode on raw pointers (the argument checks run before any device work)."""
        n = len(wav_ptrs)
        lib = _e.load_library()
        h = self.handle(finalize)
        wp, L, op = ptr_array(wav_ptrs), i32_array(lengths), ptr_array(out_ptrs)
        stream = _e.current_stream_ptr(self.device) if self.device.type == "cuda" else None
        _e._check(lib.vx_codec_encode(h, n, wp, L, n_q, op, stream))

    def last_embeddings(self, frames: int) -> torch.Tensor:
        """(frames, hidden) float32: the quantiser's input of the last encode call, its utterances concatenated (parity tests)."""
        out = torch.empty((frames, self.cfg.hidden), dtype=torch.float32, device=self.device)
        _e._check(_e.load_library().vx_codec_last_embeddings(self.handle(), out.data_ptr(), frames, _e.current_stream_ptr(self.device)))
        return out

    def encode(self, wav: torch.Tensor, n_q: Optional[int] = None, sr: Optional[int] = None) -> torch.Tensor:
        """(1, 1, L), (1, L) or (L,) float32 -> (1, n_q, ceil(L / hop)) int64 on the device; `sr` as in `encode_batch`."""
        return self.encode_batch([wav], n_q, sr)[0]

    @torch.no_grad()
    def roundtrip_mel_distance(self, wav: torch.Tensor, n_q: Optional[int] = None, sr: Optional[int] = None) -> torch.Tensor:
        """Mean absolute log-mel difference between a waveform and decode(encode(waveform)), a 0-dim tensor on the device: the
        check to run after `load_state_dict` with trained weights (a codec that reproduces speech stays well below 1; on
        synthetic weights the number means nothing).  `wav` and `sr` as in `encode`; the comparison is at 24 kHz, against the
        mixed-down and resampled input.  Needs `encoder=True`."""
        from .fbank import mel_distance

        wav = to_native_rate(self, [wav], sr, SAMPLE_RATE)[0]
        rec = self.decode(self.encode(wav, n_q))
        a, b = self.fbank().extract_batch([wav, rec])
        return mel_distance(a, b)

    @torch.no_grad()
    def roundtrip_mstft(self, wav: torch.Tensor, n_q: Optional[int] = None, sr: Optional[int] = None):
        """The multi-resolution STFT distance (`stft.MSTFTResult`: sc, log_mag per resolution, total) of decode(encode(waveform))
        against the waveform, over their common length: what `roundtrip_mel_distance` averages away at its one framing (pre-echo at
        the 240-sample window, smearing at the 1200-sample one).  `wav` and `sr` as in `encode`; the comparison is at 24 kHz,
        against the mixed-down and resampled input, which must keep 1025 samples.  On synthetic weights the number means nothing.
        Needs `encoder=True`."""
        from .stft import shared_mstft

        wav = to_native_rate(self, [wav], sr, SAMPLE_RATE)[0]
        rec = self.decode(self.encode(wav, n_q))
        return shared_mstft(rec.device).compare(rec.reshape(-1), wav.reshape(-1))

    @torch.no_grad()
    def roundtrip_speaker_similarity(self, wav: torch.Tensor, encoder, n_q: Optional[int] = None, sr: Optional[int] = None,
                                     normalize: bool = False) -> torch.Tensor:
        """The speaker similarity (`spk.SpeakerEncoder`: the cosine of the two x-vectors, a 0-dim tensor on the device) of
        decode(encode(waveform)) against the waveform: whether the codec keeps the voice, which the mel and M-STFT round trips do
        not say.  `wav` and `sr` as in `encode`; both sides go to the encoder at 24 kHz and are resampled to 16 kHz there.  On
        synthetic weights (the codec's or the encoder's) the number means nothing.  Needs `encoder=True`."""
        wav = to_native_rate(self, [wav], sr, SAMPLE_RATE)[0]
        rec = self.decode(self.encode(wav, n_q))
        return encoder.similarity(wav.reshape(-1), rec.reshape(-1), sr=SAMPLE_RATE, normalize=normalize)[0]

    def roundtrip_wer(self, wav: torch.Tensor, text: str, recognizer, n_q: Optional[int] = None, sr: Optional[int] = None,
                      normalize: bool = False, unit: str = "word"):
        """The word error rate (`asr.recognition_error`, an `asr.ErrorRate`; `unit="char"`: the character error rate) of
        decode(encode(waveform)) against `text`, what the waveform says: whether the codec keeps the words.  `wav` and `sr` as in
        `encode`; the reconstruction goes to the recogniser at 24 kHz and is resampled to 16 kHz there.  On synthetic weights (the
        codec's or the recogniser's) the number means nothing.  Needs `encoder=True`."""
        from .asr import recognition_error

        wav = to_native_rate(self, [wav], sr, SAMPLE_RATE)[0]
        rec = self.decode(self.encode(wav, n_q))
        return recognition_error(text, rec.reshape(-1), recognizer, sr=SAMPLE_RATE, normalize=normalize, unit=unit)

    def roundtrip_text_likelihood(self, wav: torch.Tensor, text: str, recognizer, n_q: Optional[int] = None, sr: Optional[int] = None,
                                  normalize: bool = False):
        """The CTC likelihood (`asr.text_likelihood`, an `asr.TextScore`: `-log p(text | audio)` and its per-character mean) of
        `text` under decode(encode(waveform)): a continuous companion of `roundtrip_wer` that still moves when the error rate is
        0 on both sides of a comparison.  Arguments as `roundtrip_wer`'s; on synthetic weights the number means nothing.  Needs
        `encoder=True`."""
        from .asr import text_likelihood

        wav = to_native_rate(self, [wav], sr, SAMPLE_RATE)[0]
        rec = self.decode(self.encode(wav, n_q))
        return text_likelihood(text, rec.reshape(-1), recognizer, sr=SAMPLE_RATE, normalize=normalize)[0]


class AudioTokenizer:
    """The reference's `valle.data.tokenizer.AudioTokenizer` (tokenizer.py:238-254) on the GPU: `encode(wav)` with wav (B, 1, L)
    returns `[(codes (B, n_q, T), None)]` as `tokenize_audio` hands it on (needs `EncodecDecoder(encoder=True)`), and
    `decode([(frames, None)])` takes frames (B, n_q, T), as `infer.py:251-253` passes `encoded_frames.transpose(2, 1)`."""

    sample_rate = 24000
    channels = 1

    def __init__(self, decoder: EncodecDecoder):
        self.decoder = decoder

    @property
    def device(self):
        return self.decoder.device

    def decode(self, frames, sr: Optional[int] = None) -> torch.Tensor:
        assert len(frames) == 1, "one (codes, scale) pair: the 24 kHz model decodes whole utterances"
        codes, scale = frames[0]
        assert scale is None, "the 24 kHz model does not normalise"
        wavs = self.decoder.decode_batch([codes[b] for b in range(codes.shape[0])], sr)
        return torch.cat(wavs, dim=0)  # (B, 1, hop T), at `sr`: (B, 1, ceil(sr hop T / 24000))

    def encode(self, wav: torch.Tensor, sr: Optional[int] = None):
        """wav (B, 1, L) at 24 kHz; with `sr` given: (B, C, L) at that rate, mixed down and resampled on the GPU."""
        if sr is None:
            assert wav.dim() == 3 and wav.shape[1] == 1, "wav is (B, 1, L): mono"
        else:
            assert wav.dim() == 3, "wav is (B, C, L)"
        codes = self.decoder.encode_batch([wav[b] for b in range(wav.shape[0])], sr=sr)
        return [(torch.cat(codes, dim=0), None)]  # every row of a (B, C, L) tensor has the same length
