"""Times qsp_essential_graph_optimize (Optimizer::OptimizeEssentialGraph on the device): one call at 50 / 200 / 1000 key frames
(ring scenes of tests/essential_oracle.make_scene: drift 0.01, three normal edges per key frame, a loop edge, one point per key
frame, n_iter = 20, lambda_init = 1e-16, scale free), 5 warm-ups, then the median and min-max of the timed calls ->
profiles/essential_graph.txt.  Also runs the parity fixtures and writes the GPU's distance from the float64 oracle beside the
oracle's own sensitivity and the bars -> profiles/essential_margins.json, and the stage scenes through qsp_essential_graph_stages ->
profiles/essential_stage_margins.json (`stages` alone does only the latter).

    python tools/time_essential.py [reps | stages]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import essential_oracle as eo                       # noqa: E402
from qsp_slam_amd.ba import essential_graph_optimize, essential_graph_stages           # noqa: E402


def call(sc):
    return essential_graph_optimize(sc["sim3"], sc["fixed"], sc["v0"], sc["v1"], sc["meas"], sc["fix_scale"], n_iter=sc["n_iter"],
                                    lambda_init=sc["lambda_init"], pts=sc["pts"], pt_ref=sc["ref"])


def stage_runs(name):
    """the device's stage outputs of a stage scene at the three dampings of essential_oracle.STAGE_LAMBDAS, and those dampings"""
    sc = eo.stage_scene(name)
    run = lambda lam: essential_graph_stages(sc["sim3"], sc["fixed"], sc["v0"], sc["v1"], sc["meas"], sc["fix_scale"], lam)
    first = run(eo.STAGE_LAMBDAS[0])
    lams = [eo.STAGE_LAMBDAS[0], 1e-5 * first["max_diag"], eo.STAGE_LAMBDAS[2]]
    return [first, run(lams[1]), run(lams[2])], lams


def stage_margins():
    gpu = {}
    for name in eo.STAGE_SCENES:
        sc = eo.stage_scene(name)
        gpu[name] = eo.stage_distance(name, *stage_runs(name))
        P, R = eo.stage_points(sc, 600)
        r = essential_graph_optimize(sc["sim3"], sc["fixed"], sc["v0"], sc["v1"], sc["meas"], sc["fix_scale"], n_iter=2, pts=P, pt_ref=R)
        gpu[name]["pt_abs"] = float(np.max(np.abs(r["pts"] - eo.correct_points(sc["sim3"], r["sim3"], P, R, longdouble=True))))
    doc = eo.write_stage_margins(gpu)
    print(json.dumps(doc["gpu_distance"], indent=1, sort_keys=True))


def main():
    if sys.argv[1:] == ["stages"]:
        return stage_margins()
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    lines = ["qsp_essential_graph_optimize, one call, host arrays in to host arrays out; ms: median (min - max) of %d calls after 5 warm-ups" % reps,
             "n_kf  n_edge  unknowns  iterations  trials   ms"]
    for n_kf in (50, 200, 1000):
        sc = eo.make_scene(1, n_kf, fixed_at=0, n_pt=n_kf, n_iter=20, drift=0.01)
        for _ in range(5):
            r = call(sc)
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            r = call(sc)
            ts.append(1e3 * (time.perf_counter() - t))
        lines.append("%4d  %6d  %8d  %10d  %6d   %.2f (%.2f - %.2f)" % (n_kf, len(sc["v0"]), 7 * (n_kf - 1), r["iters"], int(r["trace"][:, 2].sum()),
                                                                      float(np.median(ts)), min(ts), max(ts)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "essential_graph.txt"), "w").write("\n".join(lines) + "\n")
    doc = json.load(open(eo.MARGINS)) if os.path.isfile(eo.MARGINS) else {}
    doc["gpu_distance"] = {name: eo.distance(call(eo.fixture(name)), eo.fixture_result(name)) for name in eo.FIXTURES}
    doc["sensitivity"] = eo.measured_sensitivity()
    doc["bar"] = {name: eo.bars(name) for name in eo.FIXTURES}
    json.dump(doc, open(eo.MARGINS, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc["gpu_distance"], indent=1, sort_keys=True))
    stage_margins()


if __name__ == "__main__":
    main()
