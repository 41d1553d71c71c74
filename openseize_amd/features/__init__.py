from openseize_amd.features.windowed import WINDOW_FEATURES, window_features  # noqa: F401
