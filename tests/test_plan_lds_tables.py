"""The plan kernels (qp_plan_kernel, ik_plan_kernel: csrc/ik4.hip; mpc_plan_kernel: csrc/mpc.hip) keep their launch-invariant tables in
LDS: the MPC's gain blocks Gr (one 64-stage pass: horizons up to N = 63; a longer one reads the global table) and the IK's per-variable
tables kq, qreg, vlo, vhi, sd, isd.  Every wave fills the block once, in its first record, and reads it where a record uses it.

Every case runs tests/helpers/plan_lds_tables_check.py in a process of its own (torch brings its own HIP runtime and has to initialise
before libwcqp's does) and compares plans with the single wcqp_mpc_solve_device / wcqp_ik_solve_device calls bit for bit (torch.equal on
every output array of every record, first launch and replay).  Shapes: the smallest at which the staging can go wrong - 5 robots are two
workgroups, one of them ragged; 3 records over 2 ways give one way a second record (which reads the block its first record filled) and
the other only a first; ways = 0 is the work queue, whose waves draw their first record behind the fill."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the Gr stage holds kGrLdsStages = 64 stages (csrc/mpc_device.h): N = 63 is the longest horizon that is staged, N = 64 the first fallback
GR_STAGES = 64


def check(*case):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "plan_lds_tables_check.py"), *map(str, case)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "plan lds tables ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("ways", [2, 0])
@pytest.mark.parametrize("form", ["qpoases", "osqp"])
def test_per_joint_solver_tables(form, ways):
    """An IK solver whose tables differ in every entry (v_min / v_max, weights - so sd and isd -, gains and posture per joint): a lane
    that reads a neighbour's entry changes the result.  The bounds are tight enough to be active (asserted in the qpoases form), so the
    outputs' exact bounds come out of the block as well."""
    check("tables", form, ways)


@pytest.mark.gpu
@pytest.mark.parametrize("horizon", [7, 50, GR_STAGES - 1, GR_STAGES, 200])
def test_horizons_around_the_gain_stage(horizon):
    """Combined, MPC-only and IK-only plans at a short horizon, the BASELINE one, the longest that fits the Gr stage, the first that
    does not (the global path, the IK's tables still staged) and the shipped N = 200 (more than one pass of the window)."""
    check("horizon", horizon)


@pytest.mark.gpu
def test_two_solver_pairs_back_to_back():
    """Two plans of two different solver pairs (weights, bounds, horizon) enqueued back to back on one stream, twice: a launch sees
    its own handle's tables."""
    check("pairs")


@pytest.mark.gpu
def test_driver_geometry_against_goldens():
    """4096 robots, 16 ways, 20 records - the launch bench.py times in the driver's form - against the single calls bit for bit and
    against the golden vectors as bench.py checks them."""
    check("driver")
