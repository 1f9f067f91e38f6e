"""The range checks of keyword arguments that ``data``, ``validation`` and ``rollout`` share; the caller words the message."""
from __future__ import annotations

from typing import Optional

import numpy as np


def _checked_int(value, lo: int, hi: Optional[int], message: str) -> int:
    """``value`` as an int when it is one (no bool) in [lo, hi] (``hi`` None: no upper bound); ValueError(message) otherwise."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < lo or (hi is not None and int(value) > hi):
        raise ValueError(message)
    return int(value)


def _checked_float(value, lo: float, hi: float, message: str, lo_open: bool = False, hi_open: bool = False) -> float:
    """``float(value)`` when it is finite and in [lo, hi] (``lo_open`` / ``hi_open`` leave that end out); ValueError(message) otherwise, also for
    a bool and for what float() does not take."""
    try:
        x = float(value)
    except (TypeError, ValueError):
        x = float("nan")
    if isinstance(value, bool) or not (np.isfinite(x) and lo <= x <= hi and not (lo_open and x == lo) and not (hi_open and x == hi)):
        raise ValueError(message)
    return x
