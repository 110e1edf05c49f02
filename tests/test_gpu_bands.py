"""GPU: closed-loop laps of the single-track and the cascaded NMPC against the reference's recorded laps
("closed-loop sanity bands"; fixture tests/golden/closed_loop_bands.json,
made by tests/golden/make_st_bands.py from experiments/data/*_ippodromo).

Every recorded single-track run on ippodromo starts from x0 = (Ux 4, s 1) and uses one of
four controller configs: horizon N = 50 / 60 x max_speed 18 / 20, mpc_dt 0.03, the
singletrack.yaml weights.  The same lap is driven here by the batched simulator
(vc_simulate: device horizon -> fp64 stagewise-Riccati SQP, csrc/st_sqp.hip -> fp64 RK4
plant with k(s)), until the reference simulator's stop rule s > L - 0.1
(simulation/racing.py:219).  The build replaces IPOPT by five SQP iterations per step
(config/singletrack_mpc.yaml `qp`), so
the laps are compared as bands, not traces (the NLP solution is not
reproducible to 1e-5 across solvers):
  * lap length within 3 % of the recorded lap of the same config (measured: 442 vs 442,
    455 vs 448, 434 vs 433, 429 vs 428 steps);
  * median Ux within 0.3 m/s; Fx inside the recorded envelope [-7876, 6055] N widened by
    5 %; |w| <= 0.4; |ey| inside the 9 m track or within 10 % of the recorded lap's max
    (the recorded N = 50 / max_speed 20 lap itself reaches 5.06 m);
  * at most one non-solved step (the first step, from the reference's random first guess
    1 + U[0, 1) of cascaded_mpc.py:72-76).
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LAP_REL = 0.03
UX_MED_ABS = 0.3


def _recorded(ctl="singletrack"):
    with open(os.path.join(GOLDEN, "closed_loop_bands.json")) as f:
        runs = json.load(f)["runs"]
    out = {}
    for r in runs:
        if r["controller"] == ctl and r["complete"]:
            key = (r["horizon"], r["max_speed"]) if ctl == "singletrack" else (r["horizon_pm"], r["max_speed"])
            out.setdefault(key, r)
    return out


REC = _recorded()
REC_CASC = _recorded("cascaded")


@pytest.mark.parametrize("N,vmax", sorted(REC))
def test_singletrack_lap_within_recorded_bands(N, vmax):
    from vcmpc.config import load_config
    from vcmpc.environment import Track
    from vcmpc.models import DynamicCar
    from vcmpc.simulation import BatchedRacingSimulator
    rec = REC[(N, vmax)]
    track = Track.load("ippodromo")
    cfg = load_config("singletrack_mpc")
    cfg["horizon"] = N
    cfg["state_constraints"]["max_speed"] = vmax
    car = DynamicCar(load_config("dynamic_car"), track, tyre="fiala")
    sim = BatchedRacingSimulator(car, cfg, track, batch=1)
    K = int(rec["steps"] * (1 + 2 * LAP_REL))
    out = sim.reset(np.array([rec["x0"]])).run(K)
    X, U = out["state_traj"][:, 0], out["action_traj"][:, 0]
    done = np.nonzero(X[:, 4] > track.length - 0.1)[0]
    assert len(done), f"no lap in {K} steps: s = {X[-1, 4]:.1f} of {track.length:.1f}"
    lap = int(done[0])  # rows logged before the stop rule fires (the recorded arrays' length)
    Xl, Ul = X[:lap], U[:lap]
    stats = dict(steps=lap, lap_time=float(Xl[-1, 7]), Ux_median=float(np.median(Xl[:, 0])),
                 Fx_min=float(Ul[:, 0].min()), Fx_max=float(Ul[:, 0].max()), ey_absmax=float(np.abs(Xl[:, 5]).max()),
                 nfail=int(out["nfail"].sum()))
    print(f"N={N} vmax={vmax}: build {stats} | recorded steps={rec['steps']} Ux_median={rec['Ux_median']:.2f} "
          f"Fx=[{rec['Fx_min']:.0f},{rec['Fx_max']:.0f}] |ey|max={rec['ey_absmax']:.2f}")
    assert abs(lap - rec["steps"]) <= LAP_REL * rec["steps"], (lap, rec["steps"])
    assert abs(stats["Ux_median"] - rec["Ux_median"]) <= UX_MED_ABS
    assert -7876 * 1.05 <= stats["Fx_min"] and stats["Fx_max"] <= 6055 * 1.05
    assert np.abs(Ul[:, 1]).max() <= 0.4 + 1e-9
    # on the track, or no further off it than the recorded lap (N = 50 / max_speed 20: 5.06 m)
    assert stats["ey_absmax"] < max(track.width / 2, 1.1 * rec["ey_absmax"])
    assert stats["nfail"] <= 1


@pytest.mark.parametrize("M,vmax", sorted(REC_CASC))
def test_cascaded_lap_within_recorded_bands(M, vmax):
    """The reference's headline controller (CascadedMPC with a point-mass tail,
    config/controllers/cascaded.yaml) on the device: N = 20 single-track + M point-mass stages
    (csrc/casc_ric.hip, fp64, 5 SQP iterations per step -- the closed-loop setting of
    singletrack_mpc.yaml), against every recorded cascaded lap config on ippodromo
    (M = 15 / 25 / 35 / 40 x max_speed 18 .. 30; recorded 418 .. 432 steps)."""
    from vcmpc.config import load_config
    from vcmpc.environment import Track
    from vcmpc.models import DynamicCar
    from vcmpc.simulation import BatchedRacingSimulator
    rec = REC_CASC[(M, vmax)]
    track = Track.load("ippodromo")
    cfg = load_config("cascaded_mpc")
    cfg["horizon"], cfg["horizon_pm"] = rec["horizon"], M
    cfg["state_constraints"]["max_speed"] = vmax
    cfg["qp"] = dict(cfg["qp"], sqp_iters=5)
    car = DynamicCar(load_config("dynamic_car"), track, tyre="fiala")
    sim = BatchedRacingSimulator(car, cfg, track, batch=1)
    K = int(rec["steps"] * (1 + 2 * LAP_REL))
    out = sim.reset(np.array([rec["x0"]])).run(K)
    X, U = out["state_traj"][:, 0], out["action_traj"][:, 0]
    done = np.nonzero(X[:, 4] > track.length - 0.1)[0]
    assert len(done), f"no lap in {K} steps: s = {X[-1, 4]:.1f} of {track.length:.1f}"
    lap = int(done[0])
    Xl, Ul = X[:lap], U[:lap]
    stats = dict(steps=lap, Ux_median=float(np.median(Xl[:, 0])), Fx_min=float(Ul[:, 0].min()),
                 Fx_max=float(Ul[:, 0].max()), ey_absmax=float(np.abs(Xl[:, 5]).max()), nfail=int(out["nfail"].sum()))
    print(f"M={M} vmax={vmax}: build {stats} | recorded steps={rec['steps']} Ux_median={rec['Ux_median']:.2f} "
          f"Fx=[{rec['Fx_min']:.0f},{rec['Fx_max']:.0f}] |ey|max={rec['ey_absmax']:.2f}")
    assert abs(lap - rec["steps"]) <= LAP_REL * rec["steps"], (lap, rec["steps"])
    assert abs(stats["Ux_median"] - rec["Ux_median"]) <= UX_MED_ABS
    assert -7876 * 1.05 <= stats["Fx_min"] and stats["Fx_max"] <= 6055 * 1.05
    assert np.abs(Ul[:, 1]).max() <= 0.4 + 1e-9
    assert stats["ey_absmax"] < max(track.width / 2, 1.1 * rec["ey_absmax"])
    assert stats["nfail"] <= 1


# Round 4: the recorded obstacle runs and shoe-track runs (closed_loop_bands.json "runs_r4",
# make_st_bands.py), each driven from its recorded x0 with its own controller config on its own
# track, obstacles as recorded.  Bars, stated before the first measurement: a completed recorded
# lap -> our lap within 4 % of its steps (3 % above was measured on ippodromo only); a race car
# the simulator stopped early (the other car finished) -> s after the same number of steps within
# 3 %; median Ux within 0.5 m/s; |ey| inside the track or within 10 % of the recorded max; at most
# max(1, 0.5 % of the steps) non-solved; and wherever the recorded run kept clear of every obstacle
# (clearance > 0), so does ours.  (race_obstacles_shoe's two recorded cars pass 1.48 m inside an
# obstacle -- the reference's barrier w ds / (dist - r - 0.1) turns negative inside and rewards
# staying there -- so no clearance bar applies to that run.)
def _runs_r4():
    with open(os.path.join(GOLDEN, "closed_loop_bands.json")) as f:
        return {r["key"]: r for r in json.load(f)["runs_r4"]}


RUNS_R4 = _runs_r4()

# Measured misses (r04, profiles/r04/pytest_gpu_r04*.log, scripts/band_settings.py), kept as expected
# failures with their numbers instead of moving the bars: the cascaded controller drives these two
# laps in the recorded number of steps (518 vs 517; 998-1001 vs 1026, i.e. faster) but with a
# different speed profile around the obstacles -- median Ux 12.2-12.5 vs 13.23 and 14.05-14.10 vs
# 13.49 m/s at 5, 10 and 40 SQP iterations alike, so more iterations do not move it.  Which lap is
# better by the reference's own objective: the reference NLP's stage cost with no
# proximal term (cascaded_mpc.py:101-179; oracle/dyn_sqp.py closed_loop_cost) summed along both executed
# laps (r05j, profiles/r05/pytest_bands_r05j.log): obstacles1_ippodromo build 1055.4 vs recorded 1046.5
# (+0.85 %: barrier 845.5 vs 841.3, time 130.75 vs 129.0 -- a slightly worse lap), obstacles_shoe build
# 2742.6 vs recorded 3670.0 (-25 %: Fx slew 1157 vs 2085, time 249.5 vs 256.25 -- a better one).
XFAIL_R4 = {
    "cascaded_obstacles1_ippodromo:cascaded": "median Ux 12.2-12.5 vs recorded 13.23 m/s (bar 0.5); lap 518 vs 517 steps; "
                                              "reference stage cost along the lap 1055.4 vs recorded 1046.5 (+0.85 %)",
    "cascaded_obstacles_shoe:cascaded": "median Ux 14.05-14.10 vs recorded 13.49 m/s (bar 0.5); lap 998-1001 vs 1026 steps; "
                                        "reference stage cost along the lap 2742.6 vs recorded 3670.0 (-25 %, the build's "
                                        "lap is cheaper by the reference's objective)",
    # the recorded car drove through the obstacle (1.48 m inside it); ours goes round it (0.95 m clear)
    "race_obstacles_shoe:singletrack": "s after 972 steps 663.4 vs recorded 687.4 m (3.5 %, bar 3 %); recorded car "
                                       "1.48 m inside an obstacle, ours 0.95 m clear of it",
}


@pytest.mark.parametrize("key", [pytest.param(k, marks=pytest.mark.xfail(reason=XFAIL_R4[k], strict=True,
                                                                                raises=AssertionError))
                                 if k in XFAIL_R4 else k for k in sorted(RUNS_R4)])
def test_recorded_obstacle_and_shoe_runs_within_bands(key):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "scripts"))
    from replay_recorded import config_for
    from vcmpc.config import load_config
    from vcmpc.environment import Track
    from vcmpc.models import DynamicCar
    from vcmpc.simulation import BatchedRacingSimulator
    rec = RUNS_R4[key]
    track = Track.load(rec["track"])
    cfg = config_for(key, rec["config"])
    if cfg.get("horizon_pm", 0):
        cfg["qp"] = dict(cfg["qp"], sqp_iters=5)
    # (with obstacles on, the controllers take at least DYN_OBS_SQP = 10 SQP iterations per step --
    # controllers/cascaded_mpc.py dyn_qp_block, added after the first measurement of these runs)
    car = DynamicCar(load_config("dynamic_car"), track, tyre="fiala")
    sim = BatchedRacingSimulator(car, cfg, track, batch=1)
    K = int(rec["steps"] * 1.08) if rec["complete"] else rec["steps"]
    out = sim.reset(np.array([rec["x0"]])).run(K)
    X, U = out["state_traj"][:, 0], out["action_traj"][:, 0]
    assert np.isfinite(X).all()
    done = np.nonzero(X[:, 4] > track.length - 0.1)[0]
    n = int(done[0]) if len(done) else K
    Xl = X[:n]
    clear = None
    if rec["obstacles"]:
        clear = float(min(np.hypot(Xl[:, 4] - o.s, Xl[:, 5] - o.ey).min() - o.radius for o in track.obstacles))
    stats = dict(steps=n, s_end=float(X[min(rec["steps"], len(X) - 1), 4]), Ux_median=float(np.median(Xl[:, 0])),
                 ey_absmax=float(np.abs(Xl[:, 5]).max()), nfail=int(out["nfail"].sum()), clearance=clear)
    print(f"{key}: build {stats} | recorded steps={rec['steps']} complete={rec['complete']} s_end={rec['s_end']:.1f} "
          f"Ux_median={rec['Ux_median']:.2f} |ey|max={rec['ey_absmax']:.2f} clearance={rec['clearance_min']}")
    if rec["obstacles"] and rec["complete"]:
        # the reference NLP's own stage cost (no prox) summed along both executed laps (oracle/dyn_sqp.py
        # closed_loop_cost): which closed loop is better by the reference's objective
        from oracle import dyn_sqp as D
        from oracle import models as M
        from replay_recorded import load_kat
        g = load_kat()
        if f"{key}/state_traj" in g:
            p = M.dyn_params_from_config(load_config("dynamic_car"))
            W = D.dyn_weights(cfg)
            obs = [(o.s, o.ey, o.radius) for o in track.obstacles]
            Xr, Ur = g[f"{key}/state_traj"], g[f"{key}/action_traj"]
            lap = int(rec["lap_steps"])
            jb = D.closed_loop_cost(X[:n + 1], U[:n + 1], 0.05, p, W, obs)
            jr = D.closed_loop_cost(Xr[:lap + 1], Ur[1:lap + 2], 0.05, p, W, obs)
            print(f"  closed-loop reference cost (lap): build {jb['total']:.2f} {jb} | recorded {jr['total']:.2f} {jr}")
    if rec["complete"]:
        assert len(done), f"no lap in {K} steps: s = {X[-1, 4]:.1f} of {track.length:.1f}"
        assert abs(n - rec["lap_steps"]) <= 0.04 * rec["lap_steps"], (n, rec["lap_steps"])
    else:
        assert abs(stats["s_end"] - rec["s_end"]) <= 0.03 * rec["s_end"], (stats["s_end"], rec["s_end"])
    assert abs(stats["Ux_median"] - rec["Ux_median"]) <= 0.5
    assert stats["ey_absmax"] < max(track.width / 2, 1.1 * rec["ey_absmax"])
    assert stats["nfail"] <= max(1, 0.005 * n)
    if rec["obstacles"] and rec["clearance_min"] > 0:
        assert clear > 0
