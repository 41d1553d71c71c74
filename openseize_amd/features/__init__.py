from openseize_amd.features.windowed import WINDOW_FEATURES, window_features  # noqa: F401
from openseize_amd.features.entropy import WINDOW_ENTROPIES, window_entropy  # noqa: F401
from openseize_amd.features.quantiles import WINDOW_QUANTILES, window_quantiles  # noqa: F401
from openseize_amd.features.spectral import WINDOW_SPECTRAL, window_spectral  # noqa: F401
from openseize_amd.features.connectivity import WINDOW_CONNECTIVITY, window_connectivity  # noqa: F401
from openseize_amd.features.fractal import WINDOW_FRACTALS, dfa_scales, window_fractal  # noqa: F401
from openseize_amd.features.wavelet import (WAVELETS, WINDOW_WAVELET, wavelet_bands, wavelet_filters,  # noqa: F401
                                            wavelet_level, window_wavelet)
from openseize_amd.features.ar import AR_METHODS, WINDOW_ARS, window_ar  # noqa: F401
from openseize_amd.features.xcorr import WINDOW_XCORR, window_xcorr, xcorr_lags  # noqa: F401
from openseize_amd.features.granger import WINDOW_GRANGER, window_granger  # noqa: F401
from openseize_amd.features.mutual_info import MI_BINNINGS, WINDOW_MI, window_mutual_info  # noqa: F401
from openseize_amd.features.transfer_entropy import WINDOW_TE, window_transfer_entropy  # noqa: F401
from openseize_amd.features.coherence import WINDOW_COHERENCE, window_coherence  # noqa: F401
