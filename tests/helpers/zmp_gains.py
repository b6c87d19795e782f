"""Scenarios for ZMP-CoM gain scheduling (the restatement is oracle/zmp_gains_spec.py and oracle/tick_spec.py::run_ticks(
zmp_gain_schedule=...)): the shipped robots' schedules and references with stance stretches."""
import numpy as np

# zmpControllerParams.ini of the three shipped robots: smoothingTime, kCoM_stance, kZMP_stance (useGainScheduling 1 on all three;
# the walking gains are tests/robots.py's k_com / k_zmp)
ZMP_SCHEDULE = {
    "iCubGazeboV2_5": dict(zmp_smoothing_time=0.05, k_com_stance=6.0, k_zmp_stance=0.9),
    "iCubGenova04": dict(zmp_smoothing_time=0.1, k_com_stance=6.0, k_zmp_stance=0.9),
    "icubGazeboSim": dict(zmp_smoothing_time=0.1, k_com_stance=5.0, k_zmp_stance=1.2),
}


def pause_reference(ref, pauses):
    """ref [B][stages][2] with robot i's reference held still over its pauses [(start, length), ...] and resumed where it stopped (a stop
    and a restart of the planned walk; the stages run out at the end).  Returns the new array and the index map."""
    B, S, _ = ref.shape
    out = np.empty_like(ref)
    idx = np.zeros((B, S), np.int64)
    for i in range(B):
        m = 0
        for s in range(S):
            held = any(a <= s < a + n for a, n in pauses.get(i, ()))
            idx[i, s] = m
            if not held:
                m = min(m + 1, S - 1)
        out[i] = ref[i, idx[i]]
    return out, idx
