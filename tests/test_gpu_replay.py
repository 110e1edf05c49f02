"""GPU: the build's SQP against the reference's own IPOPT solutions.  Open-loop replay of
recorded closed-loop runs (tests/golden/replay_kat/, make_replay_kat.py): at every
recorded control step the drop-in controller gets the recorded state (its own previous
solution as the unshifted warm start, cascaded_mpc.py:320-321), and its first input is
compared with the command IPOPT produced from that state (action_traj[n + 1]: racing.py:77-84
logs a zero action first, then the command from state_traj[n] at :230-237), its plan with
IPOPT's recorded plan (get_state_prediction, racing.py:239-240).

The SQP's fixed point is a KKT point of the reference NLP (the Gauss-Newton model and the
proximal term vanish at a fixed point, the frozen if_else branches match), so with enough
SQP iterations the two solvers agree wherever they find the same local optimum.  Measured
(scripts/replay_recorded.py, profiles/r02/replay.json): single-track N = 60 with 40 SQP
iterations, median |dFx| 2e-5 N of |Fx| <= 6055 N and median |dw| < 1e-6; cascaded 20 + 40
converges more slowly (median |dFx| 241 / 109 / 63 / 24 N at 5 / 10 / 20 / 40 iterations).
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "scripts"))
    from replay_recorded import load_kat
    return load_kat()


def _replay(data, run, sqp, qp=None):
    from replay_recorded import replay
    recs = json.loads(str(data["configs"]))
    return replay(run, data, recs[run], sqp, qp=qp)


def test_singletrack_replay_matches_ipopt(data):
    """singletrack_ippodromo (config/controllers/singletrack.yaml: N = 60), 428 steps."""
    r = _replay(data, "singletrack_ippodromo", 40)
    print(json.dumps({k: v for k, v in r.items() if k != "example_plan"}))
    assert r["nonsolved"] == 0 and r["nonfinite_steps"] == 0
    assert r["plan_nan_steps"] == 0
    assert r["dFx_median"] < 0.01          # N (measured 2e-5)
    assert r["dw_median"] < 1e-5           # rad/s
    assert r["frac_within_1pct"] > 0.8      # measured 0.88
    assert r["plan_dev_median_m"] < 1e-4    # global x, y over the first 20 stages
    assert r["plan_dev_p90_m"] < 0.02


def test_cascaded_replay_converges_to_ipopt(data):
    """cascaded7_ippodromo (cascaded.yaml's N = 20 + M = 40 shape and weights), 413 steps, with
    the converged SQP setting (prox 0.01, 40 SQP iterations; the bench / closed-loop setting is
    prox 0.1, 3-5 iterations): the median step matches IPOPT's command to ~1 N.  Round 3's sweep
    (profiles/r03/replay_r03d.json): prox 0.1 / 0.03 / 0.01 / 0.003 at 40 iterations give median
    |dFx| 24 / 9.2 / 1.2 / 2.7 N; the p90 (~400 N at every setting) comes from contiguous
    stretches (e.g. steps 15-21, 192-203, 306-337) where the SQP and IPOPT settle in different
    local optima of the nonconvex NLP (IPOPT at the front-tyre force bound with little steering,
    the SQP steering more and pulling less), which more iterations do not change."""
    r10 = _replay(data, "cascaded7_ippodromo", 10, qp={"prox": 0.01})
    r40 = _replay(data, "cascaded7_ippodromo", 40, qp={"prox": 0.01})
    for r in (r10, r40):
        print(json.dumps({k: v for k, v in r.items() if k != "example_plan"}))
    assert r10["nonsolved"] == 0 and r40["nonsolved"] == 0
    assert r10["nonfinite_steps"] == 0 and r40["nonfinite_steps"] == 0
    assert r40["plan_nan_steps"] == 0 and r10["plan_nan_steps"] == 0   # our plans are finite
    assert r40["dFx_median"] < 0.1 * r10["dFx_median"]
    assert r40["dFx_median"] < 2.0          # N (measured 1.22 of |Fx| <= 6055)
    assert r40["dw_median"] < 1e-4          # measured 4.3e-5
    assert r40["frac_within_1pct"] > 0.5    # measured 0.53
    assert r40["plan_dev_median_m"] < 1e-3  # measured 2.7e-4 m


# Round 4: every recorded run with the obstacle barrier on, and the shoe-track runs (fixture keys
# "<dir>:<controller>", tests/golden/make_replay_kat.py; the three giant-obstacle runs are not
# replayable: their obstacle set was never recorded).  Converged setting (prox 0.01, 40 SQP
# iterations), the run cut into windows replayed side by side (scripts/replay_recorded.py
# replay(segments=)): each window starts from the controller's own initial guess and its first 5
# steps are not compared.  Bars, stated before the first measurement (from the two ippodromo
# runs above): single-track -- at most 1 % of the steps non-solved, median |dFx| < 1 N, median
# |dw| < 1e-4 rad/s, > 60 % of the steps within 1 %, median plan deviation < 0.01 m; cascaded
# (the slower-converging tail) -- at most 1 % non-solved, median |dFx| < 20 N, median |dw| < 1e-3,
# > 25 % within 1 %, median plan deviation < 0.05 m.  Every plan finite.
REPLAY_R4 = ["singletrack_obstacles_shoe:singletrack", "race_obstacles_shoe:singletrack", "singletrack_shoe:singletrack",
             "race1_shoe:singletrack", "race2_shoe:singletrack",
             "cascaded_obstacles1_ippodromo:cascaded", "cascaded_obstacles2_ippodromo:cascaded",
             "cascaded_obstacles_shoe:cascaded", "race_obstacles_shoe:cascaded", "race1_shoe:cascaded",
             "race2_shoe:cascaded"]


# Measured misses.  race_obstacles_shoe's recorded cars drive 1.48 m *inside* an obstacle (the reference's
# barrier w ds / (dist - r - 0.1) turns negative there); replayed from those states with the build's
# default barrier (finite below its 0.05 m margin floor).  Round 6 (r06e, profiles/r06/
# replay_r06e.json; ABI 12 status VC_OUT_OF_DOMAIN, neutral restart after a failed retry): single-track 4 of
# 851 steps non-solved (1 max_iter, 3 out of the model's domain -- round 5 returned those as solved and
# the next step's ds went non-finite), median |dFx| 0.57 N, 56.2 % within 1 % (bar 60 %); cascaded 0
# non-solved, median |dFx| 21.4 N (bar 20 N), 46.5 % within 1 %.  Strict: an exception is not a miss.
XFAIL_REPLAY_R4 = {"race_obstacles_shoe:singletrack": "r06e: 4 of 851 non-solved (1 max_iter, 3 out of domain), median |dFx| "
                                                      "0.57 N, 56.2 % of the steps within 1 % (bar 60 %)",
                   "race_obstacles_shoe:cascaded": "r06e: 0 of 851 non-solved, median |dFx| 21.4 N (bar 20 N), 46.5 % within "
                                                   "1 %; with the reference's own barrier inside (vc_obstacles.inside) it passes "
                                                   "every bar (6.8 N, 49.1 %)"}


@pytest.mark.parametrize("run", [pytest.param(r, marks=pytest.mark.xfail(reason=XFAIL_REPLAY_R4[r], strict=True,
                                                                                 raises=AssertionError))
                                 if r in XFAIL_REPLAY_R4 else r for r in REPLAY_R4])
def test_replay_obstacle_and_shoe_runs(data, run):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "scripts"))
    from replay_recorded import replay
    recs = json.loads(str(data["configs"]))
    r = replay(run, data, recs[run], 40, qp={"prox": 0.01}, segments=24)
    print(json.dumps({k: v for k, v in r.items() if k != "example_plan"}))
    casc = run.endswith(":cascaded")
    assert r["nonfinite_steps"] == 0        # u0, the plan and the next warm start finite at every step
    assert r["plan_nan_steps"] == 0
    assert r["nonsolved"] <= 0.01 * r["steps"]
    assert r["dFx_median"] < (20.0 if casc else 1.0)
    assert r["dw_median"] < (1e-3 if casc else 1e-4)
    assert r["frac_within_1pct"] > (0.25 if casc else 0.6)
    assert r["plan_dev_median_m"] < (0.05 if casc else 0.01)


# Round 5: every remaining recorded horizon shape (tests/golden/make_replay_kat.py) -- single-track
# N = 50 (race1_ippodromo, BASELINE.md's first row: 431 recorded IPOPT commands) and the cascaded
# tails M = 15 / 25 / 35 (race1/2/3_ippodromo).  Same converged setting, windows and bars as the
# round-4 runs above, stated before measuring: single-track <= 1 % non-solved, median |dFx| < 1 N,
# median |dw| < 1e-4, > 60 % within 1 %, median plan deviation < 0.01 m; cascaded <= 1 %, < 20 N,
# < 1e-3, > 25 %, < 0.05 m; every plan finite.
REPLAY_R5 = ["race1_ippodromo:singletrack", "race1_ippodromo:cascaded", "race2_ippodromo:cascaded",
             "race3_ippodromo:cascaded"]


@pytest.mark.parametrize("run", REPLAY_R5)
def test_replay_every_recorded_horizon_shape(data, run):
    test_replay_obstacle_and_shoe_runs(data, run)


# Round 5: race_obstacles_shoe with the reference's own barrier inside the obstacle (vc_obstacles.inside,
# ABI 11): the recorded cars drive 1.48 m inside an obstacle, where the reference's barrier
# w ds / (dist - r - 0.1) is negative and the build's default floors the margin at 0.05 m.  With the
# inside mode the QP model equals the reference's barrier everywhere except the band |margin| <= 0.05 m.
# Bars: the round-4 ones above, stated before this measurement.
# Measured (r06e, profiles/r06/replay_inside_r06e.json): cascaded passes every bar (0 of 851 non-solved, median
# |dFx| 6.8 N, 49.1 % within 1 %); single-track 4 of 851 non-solved and every bar but one: 57.0 % of the steps
# within 1 % of IPOPT's command against the 60 % stated before measuring -- kept as an expected failure
# (strict: an exception is not a miss; round 5's run crashed here on a non-finite horizon).
@pytest.mark.parametrize("run", [pytest.param("race_obstacles_shoe:singletrack", marks=pytest.mark.xfail(
    reason="r06e: 4 of 851 non-solved, median |dFx| 0.56 N, but 57.0 % of the steps within 1 % (bar 60 %)", strict=True,
    raises=AssertionError)),
    "race_obstacles_shoe:cascaded"])
def test_replay_race_obstacles_shoe_reference_barrier(data, run):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "scripts"))
    from replay_recorded import replay
    recs = json.loads(str(data["configs"]))
    r = replay(run, data, recs[run], 40, qp={"prox": 0.01}, segments=24, cfg_extra={"obstacle_inside": True})
    print(json.dumps({k: v for k, v in r.items() if k != "example_plan"}))
    casc = run.endswith(":cascaded")
    assert r["nonfinite_steps"] == 0        # u0, the plan and the next warm start finite at every step
    assert r["plan_nan_steps"] == 0
    assert r["nonsolved"] <= 0.01 * r["steps"]
    assert r["dFx_median"] < (20.0 if casc else 1.0)
    assert r["dw_median"] < (1e-3 if casc else 1e-4)
    assert r["frac_within_1pct"] > (0.25 if casc else 0.6)
    assert r["plan_dev_median_m"] < (0.05 if casc else 0.01)


# Round 6: the 24 remaining replayable recorded controller runs (tests/golden/make_replay_kat.py; VERDICT r05
# missing 1).  Their horizon shapes are all covered above, but each carries its own max_speed cap
# (18 / 20 / 26 / 30 m/s), slip-angle weights and recorded trajectory.  Same converged setting and windows
# as the round-4/5 runs; bars stated before measuring, the round-4/5 ones: single-track <= 1 % of the steps
# non-solved, median |dFx| < 1 N, median |dw| < 1e-4 rad/s, > 60 % of the steps within 1 % of IPOPT's
# command, median plan deviation < 0.01 m; cascaded <= 1 %, < 20 N, < 1e-3, > 25 %, < 0.05 m; every
# output and warm start finite.
REPLAY_R6 = ["singletrack2_ippodromo:singletrack", "singletrack3_ippodromo:singletrack",
             "singletrack4_ippodromo:singletrack", "singletrack_slip_angle_ippodromo:singletrack",
             "singletrack_slip_angle2_ippodromo:singletrack", "singletrack_slip_angle3_ippodromo:singletrack",
             "cascaded1_ippodromo:cascaded", "cascaded2_ippodromo:cascaded", "cascaded3_ippodromo:cascaded",
             "cascaded4_ippodromo:cascaded", "cascaded5_ippodromo:cascaded", "cascaded6_ippodromo:cascaded",
             "cascaded_slip_angle_ippodromo:cascaded", "cascaded_slip_angle2_ippodromo:cascaded",
             "race2_ippodromo:singletrack", "race3_ippodromo:singletrack",
             "race4_ippodromo:singletrack", "race4_ippodromo:cascaded", "race5_ippodromo:singletrack",
             "race5_ippodromo:cascaded", "race6_ippodromo:singletrack", "race6_ippodromo:cascaded",
             "race7_ippodromo:singletrack", "race7_ippodromo:cascaded"]


@pytest.mark.parametrize("run", REPLAY_R6)
def test_replay_remaining_recorded_runs(data, run):
    test_replay_obstacle_and_shoe_runs(data, run)
