"""MI355X-native VALL-E inference engine (drop-in for ``valle.models.VALLE.inference``)."""
from .config import ModelConfig, add_model_arguments, NUM_AUDIO_TOKENS, NUM_TEXT_TOKENS  # noqa: F401


__all__ = ["ModelConfig", "add_model_arguments", "NUM_AUDIO_TOKENS", "NUM_TEXT_TOKENS", "AudioTokenizer", "CodecConfig", "EncodecDecoder",
           "Resampler", "convert_audio", "load_wav", "save_wav", "tokenize_audio",
           "BigVGANFbank", "BigVGANFbankConfig", "get_fbank_extractor", "mel_distance", "slaney_mel_basis",
           "DTW", "DTWResult", "mel_cepstral_distortion", "GriffinLim", "mel_to_waveform",
           "GanVocoder", "BigVGAN", "PitchTracker", "PitchTrack", "F0Result", "f0_distance",
           "STFTConfig", "MultiResolutionSTFT", "MSTFTResult", "mstft_distance", "copy_synthesis_distance",
           "SpeakerEncoder", "SpeakerConfig", "speaker_similarity",
           "SpeechRecognizer", "RecognizerConfig", "Transcript", "ErrorRate", "edit_distance", "word_error_rate", "char_error_rate",
           "recognition_error", "TextAlignment", "TextScore", "ctc_forced_align", "ctc_nll", "text_likelihood",
           "WhisperRecognizer", "WhisperConfig", "WhisperTranscript"]


def __getattr__(name):  # the codec pulls in torch and the ctypes binding: imported on first use, not with the package
    if name in ("AudioTokenizer", "CodecConfig", "EncodecDecoder", "Resampler", "convert_audio", "load_wav", "save_wav", "tokenize_audio"):
        from . import codec

        return getattr(codec, name)
    if name in ("BigVGANFbank", "BigVGANFbankConfig", "get_fbank_extractor", "mel_distance", "slaney_mel_basis"):
        from . import fbank

        return getattr(fbank, name)
    if name in ("DTW", "DTWResult", "mel_cepstral_distortion"):
        from . import dtw

        return getattr(dtw, name)
    if name in ("GriffinLim", "mel_to_waveform"):
        from . import vocoder

        return getattr(vocoder, name)
    if name in ("GanVocoder", "BigVGAN"):
        from . import ganvoc

        return getattr(ganvoc, name)
    if name in ("PitchTracker", "PitchTrack", "F0Result", "f0_distance"):
        from . import pitch

        return getattr(pitch, name)
    if name in ("STFTConfig", "MultiResolutionSTFT", "MSTFTResult", "mstft_distance", "copy_synthesis_distance"):
        from . import stft

        return getattr(stft, name)
    if name in ("SpeakerEncoder", "SpeakerConfig", "speaker_similarity"):
        from . import spk

        return getattr(spk, name)
    if name in ("SpeechRecognizer", "RecognizerConfig", "Transcript", "ErrorRate", "edit_distance", "word_error_rate", "char_error_rate",
                "recognition_error", "TextAlignment", "TextScore", "ctc_forced_align", "ctc_nll", "text_likelihood"):
        from . import asr

        return getattr(asr, name)
    if name in ("WhisperRecognizer", "WhisperConfig", "WhisperTranscript"):
        from . import whisper

        return getattr(whisper, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
