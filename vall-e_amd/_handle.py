"""What every wrapper of a C handle (`vx_<prefix>_create` ... `vx_<prefix>_destroy`, include/vallex.h) shares: the life of the handle, the
call on it, the hand-over of weights, the preparation of waveforms and the process-wide objects per device.  Private: the public
names stay in their modules.  A new front-end starts from `Handle` (with weights: `WeightedHandle`), gives `_PREFIX`, `_NAME` and
`_config_struct()`, and writes its `_*_raw` methods as the arrays and one `_invoke`."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch

from . import engine as _e


def normalize_device(device) -> torch.device:
    """`cuda` is `cuda:<current>`: two spellings of one device compare equal afterwards."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def ptr_array(ptrs):
    """A list of addresses -> a C array of `void *`; None stays None (the C side answers a null array itself)."""
    return None if ptrs is None else (C.c_void_p * len(ptrs))(*ptrs)


def i32_array(xs):
    return None if xs is None else (C.c_int32 * len(xs))(*xs)


class Handle:
    """The handle behind the C entry points `<_PREFIX>_*`; `_NAME` is the class name the messages carry.  It is created on the host
    at construction (`_init_handle`), bound to the device of its first call, where the C side keeps its tables and workspace, and
    made again on the first call after a `.to()` to another device."""
    _PREFIX = ""
    _NAME = ""

    def _init_handle(self):
        self.device = torch.device("cpu")
        self._h = None
        self._bound = None  # the device of the handle's first call
        self._resamplers: Dict[tuple, object] = {}
        self._handle()      # what the C side does not serve is refused here

    def _fn(self, name: str):
        return getattr(_e.load_library(), f"{self._PREFIX}_{name}")

    def _create_call(self, lib, out_handle) -> int:
        return self._fn("create")(C.byref(self._config_struct()), out_handle)

    def _configure(self, lib):
        """Runs on the new `self._h` before it is handed out (tables, filters); raising destroys the handle."""

    def _upload(self):
        pass

    def _handle(self):
        if self._h is None:
            lib = _e.load_library()
            h = C.c_void_p()
            _e._check(self._create_call(lib, C.byref(h)))
            self._h, self._bound = h, None
            try:
                self._configure(lib)
                self._upload()
            except Exception:
                self.close()
                raise
        return self._h

    def to(self, device):
        self.device = normalize_device(device)
        if self._bound is not None and self._bound != self.device:
            self.close()  # another device gets a fresh handle on its first call
        return self

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._fn("destroy")(self._h)
            self._h = self._bound = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _need_device(self, what: Optional[str] = None):
        if self.device.type != "cuda":
            name = self._NAME + ("." + what if what else "")
            raise RuntimeError(f"valle_amd.{name} runs only on an MI355X: call .to('cuda') first (no CPU fallback)")

    def _invoke(self, fn, *args):
        """`fn(handle, *args, stream)`, `fn` a name under `_PREFIX` or the C function itself: the stream is read now, the first call
        on a GPU binds the handle to it, a return code other than VX_OK raises."""
        cuda = self.device.type == "cuda"
        stream = _e.current_stream_ptr(self.device) if cuda else None
        h = self._handle()
        if cuda:
            self._bound = self.device
        _e._check((self._fn(fn) if isinstance(fn, str) else fn)(h, *args, stream))


class WeightedHandle(Handle):
    """A handle that takes named tensors between create and `finalize`.  `_weights` (canonical key -> fp32 CPU tensor) is kept, so a
    handle made again for another device gets them again."""

    def _init_handle(self):
        self._weights: Optional[Dict[str, torch.Tensor]] = None
        super()._init_handle()

    def _tensors(self):
        return self._weights.items()

    def _upload(self):
        if self._weights is not None:
            for k, t in self._tensors():
                shape = (C.c_int64 * t.dim())(*t.shape)
                _e._check(self._fn("set_weight")(self._h, k.encode(), t.data_ptr(), shape, t.dim()))
            _e._check(self._fn("finalize")(self._h))

    def _need_weights(self):
        if self._weights is None:
            raise RuntimeError(f"{self._NAME} has no weights: call load_state_dict first")

    def _checked(self, want: Dict[str, tuple], w: dict, optional=(), together=()) -> Dict[str, torch.Tensor]:
        """`w` holds exactly the keys of `want` in their shapes (and any of `optional`, those of `together` all or none), else
        KeyError / ValueError by name -> the tensors as fp32 on the host."""
        missing = sorted(k for k in want if k not in w)
        unexpected = sorted(k for k in w if k not in want and k not in optional)
        if missing or unexpected:
            raise KeyError(f"{self._NAME}.load_state_dict: missing keys {missing}, unexpected keys {unexpected}")
        if len({k in w for k in together}) > 1:
            raise KeyError(f"{self._NAME}.load_state_dict: {' and '.join(together)} come together")
        for k, shape in want.items():
            if tuple(w[k].shape) != tuple(shape):
                raise ValueError(f"{self._NAME}.load_state_dict: {k} is {tuple(w[k].shape)}, expected {tuple(shape)}")
        keys = list(want) + [k for k in optional if k in w]
        return {k: w[k].detach().to("cpu", torch.float32).contiguous() for k in keys}

    def _set_weights(self, weights: Dict[str, torch.Tensor]):
        """Keeps the weights and makes the handle again with them.  Returns self."""
        self._weights = weights
        self.close()
        self._handle()
        return self

    def _check_state_dict(self, want: Dict[str, tuple], w: dict):
        return self._set_weights(self._checked(want, w))


# ---- waveforms -------------------------------------------------------------------------------------------------------------------
def owner_resampler(owner, orig_hz: int, new_hz: int):
    """The owner's `Resampler` for a rate pair, on the owner's device: kept per pair in `owner._resamplers`, `owner.max_batch`
    utterances per call.  `Resampler.to` rebinds lazily, so the owner's own `to()` has nothing to close."""
    from .codec import Resampler

    key = (int(orig_hz), int(new_hz))
    if key not in owner._resamplers:
        owner._resamplers[key] = Resampler(key[0], key[1], owner.max_batch)
    return owner._resamplers[key].to(owner.device)


def to_native_rate(owner, wavs, sr: Optional[int], native: int):
    """With `sr` given, and the rate not `native` or an entry not mono: (L,), (C, L) or (1, C, L) at `sr` -> (1, 1, L') at `native`
    through the owner's `Resampler` (at the native rate: the channel mean alone), `owner.max_batch` per call.  Else as given."""
    wavs = list(wavs)
    if sr is None or (int(sr) == native and all(w.numel() == w.shape[-1] for w in wavs)):
        return wavs
    rs, mb = owner_resampler(owner, sr, native), owner.max_batch
    return [r for i in range(0, len(wavs), mb) for r in rs.resample_batch(wavs[i:i + mb])]


def prepare_waveforms(owner, wavs, sr: Optional[int], native: int, strict: bool, what: Optional[str] = None) -> List[torch.Tensor]:
    """`to_native_rate`, then one mono float32 utterance per entry -> flat contiguous tensors on the owner's device.  `strict`: an
    entry on another device raises (nothing is moved); else it is moved.  `what` names an entry in the messages ("utterance")."""
    out = []
    for i, w in enumerate(to_native_rate(owner, wavs, sr, native)):
        assert isinstance(w, torch.Tensor) and w.dtype == torch.float32 and w.numel() == w.shape[-1], \
            (f"{what} {i}: " if what else "") + "one mono float32 waveform per entry"
        if strict and w.device != owner.device:
            raise RuntimeError(f"valle_amd.{owner._NAME}: {what} {i} is on {w.device}, the object on {owner.device} (no CPU fallback)")
        out.append(w.detach().reshape(-1).to(owner.device).contiguous())
    return out


# ---- process-wide objects ----------------------------------------------------------------------------------------------------------
def shared(cache: dict, device, key: tuple, make, module: Optional[str] = None):
    """`cache[(device,) + key]`, made by `make().to(device)` on first use.  With `module` a device that is no GPU is refused in that
    module's name."""
    device = torch.device(device)
    if module is not None and device.type != "cuda":
        raise RuntimeError(f"valle_amd.{module} runs only on an MI355X: pass device tensors (no CPU fallback)")
    key = (normalize_device(device),) + tuple(key)
    if key not in cache:
        cache[key] = make().to(key[0])
    return cache[key]
