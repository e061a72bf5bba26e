"""joeys2t_amd — MI355X-native hot path of JoeyS2T (speech-to-text), behind the reference's Python API.

Everything numeric runs in hand-written HIP kernels for gfx950 (libjoeys2t_hip.so, C ABI in
include/joeys2t_hip.h).  PyTorch provides device memory, streams, autograd routing and torch.distributed.
"""
__version__ = "0.1.0"

_LONG_FORM = ("plan_windows", "stitch_posteriors", "segment", "decode_stream", "transcribe_long", "align_long", "spot_long")  # joeys2t_amd.long_form: one recording to text
_STREAMING = ("CTCStreamDecoder", "StreamingTranscriber")  # joeys2t_amd.streaming: captions while the audio arrives
__all__ = ["long_form", *_LONG_FORM, "streaming", *_STREAMING]


def __getattr__(name):  # on first use: importing the package stays free of torch and of the library
    for module_name, names in (("long_form", _LONG_FORM), ("streaming", _STREAMING)):
        if name == module_name or name in names:
            import importlib
            module = importlib.import_module(f"joeys2t_amd.{module_name}")
            return module if name == module_name else getattr(module, name)
    raise AttributeError(f"module 'joeys2t_amd' has no attribute '{name}'")
