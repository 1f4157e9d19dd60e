"""filterpy_amd.memory -- the fading-memory polynomial filter (filterpy/memory/__init__.py)."""
from .fading_memory import FadingMemoryFilter  # noqa: F401
