"""filterpy_amd.gh -- the g-h / g-h-k filters and their gain-selection helpers (filterpy/gh/__init__.py)."""
from .gh_filter import (GHFilter, GHKFilter, GHFilterOrder, optimal_noise_smoothing,  # noqa: F401
                        least_squares_parameters, critical_damping_parameters, benedict_bornder_constants)
