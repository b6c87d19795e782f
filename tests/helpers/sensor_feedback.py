"""Readings for the tick pipeline's sensor feedback (the restatement is oracle/sensor_spec.py)."""
import numpy as np


def wrenches(rng, B, left_fz=None, right_fz=None):
    """Sole wrenches [B][6] each: normal forces of a standing robot (about 300 N between the feet) and small moments, so that each foot's
    ZMP lies within a few cm of its sole origin.  left_fz / right_fz: override the normal forces ([B] arrays)."""
    out = []
    for fz in (left_fz, right_fz):
        w = np.zeros((B, 6))
        w[:, 0:2] = rng.normal(scale=5.0, size=(B, 2))
        w[:, 2] = rng.uniform(100.0, 250.0, size=B) if fz is None else fz
        w[:, 3:5] = rng.normal(scale=3.0, size=(B, 2))
        w[:, 5] = rng.normal(scale=0.5, size=B)
        out.append(w)
    return out
