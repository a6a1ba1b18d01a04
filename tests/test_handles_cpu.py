"""No GPU: the one contract of every wrapper of a C handle (valle_amd/_handle.py), over all ten classes.

* the handle exists after construction and is bound to no device; `.to()` on a handle that was never used keeps it, whatever the
  device; a handle bound to a device is kept by `.to()` of that device and dropped by `.to()` of another, and `_handle()` makes it
  again; `close()` twice is harmless;
* without a GPU the public batch call raises the "runs only on an MI355X ... (no CPU fallback)" RuntimeError naming the class;
* every class derives from the one base: a front-end with a life cycle of its own fails here."""
import pytest
import torch

import asr_cases as AC
import ganvoc_ref as GR
import spk_cases as SC
import whisper_cases as WC


@pytest.fixture(scope="module", autouse=True)
def lib():
    import __graft_entry__ as ge

    ge.build()


def _resampler():
    from valle_amd.codec import Resampler

    return Resampler(48000, 24000, max_batch=2), lambda o: o.resample_batch([torch.zeros(2, 480)])


def _fbank():
    from valle_amd.fbank import BigVGANFbank

    return BigVGANFbank(max_batch=2), lambda o: o.extract_batch([torch.zeros(1000)])


def _griffinlim():
    from valle_amd.vocoder import GriffinLim

    return GriffinLim(max_batch=2, max_total_frames=64), lambda o: o.synthesize_batch([torch.zeros(4, 100)])


def _ganvoc():
    from valle_amd.ganvoc import GanVocoder

    cfg = GR.GEOMETRIES["g1_snakebeta"]
    return GanVocoder(cfg, max_batch=2, max_total_frames=50), lambda o: o.synthesize_batch([torch.zeros(4, cfg["n_mels"])])


def _dtw():
    from valle_amd.dtw import DTW

    return DTW(dim=8, n_ceps=0, max_frames=16, max_batch=2), lambda o: o.compare_batch([(torch.zeros(3, 8), torch.zeros(4, 8))])


def _pitch():
    from valle_amd.pitch import PitchTracker

    return PitchTracker(max_frames=10, max_batch=2), lambda o: o.track_batch([torch.zeros(1000)])


def _stft():
    from valle_amd.stft import MultiResolutionSTFT, STFTConfig

    return MultiResolutionSTFT(STFTConfig(max_samples=5000), max_batch=2), lambda o: o.compare_batch([torch.zeros(3000)], [torch.zeros(3000)])


def _spk():
    from valle_amd.spk import SpeakerEncoder

    return SpeakerEncoder(SC.config("tiny_wavlm"), max_batch=1, max_seconds=1.0), lambda o: o.embed([torch.zeros(8000)], sr=16000)


def _asr():
    from valle_amd.asr import SpeechRecognizer

    return (SpeechRecognizer(AC.config("tiny_layer"), AC.vocab("tiny_layer"), max_batch=1, max_seconds=1.0),
            lambda o: o.recognize([torch.zeros(8000)], sr=16000))


def _whisper():
    from valle_amd.whisper import WhisperRecognizer

    return WhisperRecognizer(WC.config("A"), max_batch=1), lambda o: o.recognize([torch.zeros(8000)], sr=16000)


MAKERS = {"Resampler": _resampler, "BigVGANFbank": _fbank, "GriffinLim": _griffinlim, "GanVocoder": _ganvoc, "DTW": _dtw,
          "PitchTracker": _pitch, "MultiResolutionSTFT": _stft, "SpeakerEncoder": _spk, "SpeechRecognizer": _asr,
          "WhisperRecognizer": _whisper}


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_life_cycle(name):
    obj, _ = MAKERS[name]()
    h = obj._h
    assert h is not None and obj._bound is None and obj.device.type == "cpu"
    assert obj.to("cuda:0") is obj and obj._h is h and obj.to("cuda:1")._h is h   # never used: nothing is bound yet
    assert obj.device == torch.device("cuda", 1) and obj._bound is None
    obj._bound = torch.device("cuda", 0)                                          # as after a first call on cuda:0
    assert obj.to("cuda:0")._h is h and obj._bound == torch.device("cuda", 0)
    assert obj.to("cuda:1")._h is None and obj._bound is None                     # another device: the handle is dropped
    assert obj._handle() is not None and obj._h is not None and obj._bound is None
    obj.close()
    assert obj._h is None and obj._bound is None
    obj.close()


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_no_cpu_fallback_names_the_class(name):
    obj, call = MAKERS[name]()
    with pytest.raises(RuntimeError, match=rf"valle_amd\.{name}\S* runs only on an MI355X: .*\(no CPU fallback\)"):
        call(obj)
    assert obj._h is not None and obj._bound is None
    obj.close()


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_one_base(name):
    from valle_amd import _handle

    obj, _ = MAKERS[name]()
    cls = type(obj)
    assert cls.__name__ == name == cls._NAME and issubclass(cls, _handle.Handle)
    for attr in ("_init_handle", "_handle", "to", "close", "__del__", "_invoke", "_need_device"):  # the life cycle is the base's own
        owners = [k.__name__ for k in cls.__mro__ if attr in vars(k)]
        assert owners == ["Handle"] or (attr == "_init_handle" and owners == ["WeightedHandle", "Handle"]), (attr, owners)
    obj.close()
