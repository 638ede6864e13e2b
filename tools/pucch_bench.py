#!/usr/bin/env python3
"""Times the PUCCH detector launch (srsgpu_pucch_detector_plan_execute) over the whole fixture plan of
tests/golden/pucch_detector.npz: its 360 Format 0 PDUs and 174 Format 1 resources (463 entries) in one plan, two PRBs
per case, 26 cases per 52-PRB x 4-port grid. Each round enqueues --launches executes back to back on one stream between
two device events and synchronises once; the figure is the round's time per launch, median over --rounds. "graph"
replays the same launches captured once. The results are checked against the reference's recorded bits and status
before timing. The reference detectors' time for the same cases on one host core comes from
tools/gen_pucch_golden.py --time. Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran-5g_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import pucch_cases as C  # noqa: E402
import srsgpu  # noqa: E402
import test_pucch_detector_gpu as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    ctx = srsgpu.Context(0)
    dev = torch.device("cuda", 0)
    _, f0, f1 = C.golden()
    placed0, placed1 = T.assign([(c["cfg"], c["words"]) for c in f0], [(c["cfg"], c["words"]) for c in f1])
    nof_grids = max(g for *_, g in placed0 + placed1) + 1
    grids = C.place([(c, w) for c, w, _ in placed0], [(c, w) for c, w, _ in placed1], 2 * T.PER_GRID, 4, nof_grids,
                    C.NAN_WORD, grid_of=lambda kind, i: (placed0 if kind == 0 else placed1)[i][2])
    plan = srsgpu.PucchDetectorPlan(ctx, [T.to_f0(c, g) for c, _, g in placed0], [T.to_f1(c, g) for c, _, g in placed1],
                                    2 * T.PER_GRID, 4, nof_grids)
    d_grids = torch.from_numpy(grids.view(np.int32)).to(dev)
    d_results = torch.zeros(32 * plan.nof_results, dtype=torch.uint8, device=dev)
    for _ in range(5):
        plan.execute(d_grids, d_results)
    torch.cuda.synchronize(dev)
    got = d_results.cpu().numpy().view(srsgpu.PUCCH_RESULT_DTYPE)
    assert np.array_equal(got["status"][: len(f0)], [c["status"] for c in f0])
    assert np.array_equal(got["status"][len(f0):], np.concatenate([c["status"] for c in f1]))

    def launches():
        for _ in range(args.launches):
            plan.execute(d_grids, d_results, torch.cuda.current_stream(dev))

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    graph.replay()
    torch.cuda.synchronize(dev)
    times = {"eager": [], "graph": []}
    for _ in range(args.rounds):
        for mode, run in (("eager", launches), ("graph", graph.replay)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            times[mode].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    out = {"format0_pdus": len(f0), "format1_resources": len(f1), "format1_entries": plan.nof_entries,
           "wavefronts": len(f0) + len(f1), "grids": nof_grids, "launches_per_round": args.launches}
    for mode, t in times.items():
        out[f"{mode}_us_per_launch"] = {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                                        "max": round(float(np.max(t)), 3)}
    print(json.dumps(out), flush=True)
    plan.close()


if __name__ == "__main__":
    main()
