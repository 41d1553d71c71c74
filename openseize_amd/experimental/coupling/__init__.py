"""Coupling estimators over analytic signals (experimental, as in the reference)."""

from openseize_amd.experimental.coupling.connectivity import (  # noqa: F401
    ANALYTIC_METHODS, analytic_connectivity)
