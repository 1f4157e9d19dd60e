"""filterpy_amd.leastsq -- the recursive least-squares polynomial filter (filterpy/leastsq/__init__.py)."""
from .least_squares import LeastSquaresFilter  # noqa: F401
