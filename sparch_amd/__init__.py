"""
sparch_amd — MI355X (gfx950) native implementation of sparch's recurrent spiking-layer
training path.  `sparch_amd.snns` mirrors the reference's `sparch.models.snns` API; the
arithmetic runs in libsparch_hip.so (hand-written HIP), reached through `_capi` (ctypes).
There is no CPU fallback: importing this package without the built library fails.
"""
from . import _capi  # noqa: F401  (fails loudly when libsparch_hip.so is missing)
from . import optim  # noqa: F401
from .functional import (augment_padded, bin_events, check_status, compute_dtype, fbank,  # noqa: F401
                         fbank_padded, flac_decode_padded, set_compute_dtype)
from .encoders import SpikeEncoder, StreamingSpikeEncoder, parse_encode  # noqa: F401
from .snns import (SNN, LIFLayer, RLIFLayer, RadLIFLayer, ReadoutLayer,  # noqa: F401
                   SpikeFunctionBoxcar, SpikeFunctionSurrogate, adLIFLayer)
from .streaming import StreamingFbank, StreamingSNN  # noqa: F401
from .streaming_ann import StreamingANN  # noqa: F401

__version__ = "0.1.0"
