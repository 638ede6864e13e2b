#!/usr/bin/env python3
"""Times the PRACH detector launch (srsgpu_prach_detector_plan_execute) over plans of 1, 16 and 80 occasions, for two
occasions of the fixture tests/golden/prach_detector.npz with fresh samples: Format 0 with N_cs = 13 (one root sequence,
64 windows, two ports) and B4 with N_cs = 0 (64 root sequences of one window, four ports, 12 combined symbols: the
worst case in workgroups). Each round enqueues --launches executes back to back on one stream between two device events
and synchronises once; the figure is the round's time per launch, median over --rounds. "graph" replays the same launches
captured once. The first occasion's result is checked against the float64 restatement before timing. The reference
detector's time for the same occasions on one host core comes from tools/gen_prach_golden.py --time. Prints one JSON
line per plan."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran-5g_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import prach_cases as C  # noqa: E402
import srsgpu  # noqa: E402

BENCH_CASES = ("f0_ncs13", "b4_12symbols")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--occasions", type=int, nargs="+", default=[1, 16, 80])
    args = ap.parse_args()
    ctx = srsgpu.Context(0)
    dev = torch.device("cuda", 0)
    by_name = {c["name"]: c for c in C.golden()[0]}
    rng = np.random.default_rng(1)
    for name in BENCH_CASES:
        base = by_name[name]
        for count in args.occasions:
            cases = [dict(base, words=C.transmit(base, [(5, 3, 6.0)], rng)) for _ in range(count)]
            words, occasions = C.place(cases)
            plan = srsgpu.PrachDetectorPlan(ctx, occasions, words.size)
            d_input = torch.from_numpy(words.view(np.int32)).to(dev)
            d_results = torch.zeros(srsgpu.PRACH_RESULT_DTYPE.itemsize * count, dtype=torch.uint8, device=dev)
            for _ in range(5):
                plan.execute(d_input, d_results)
            torch.cuda.synchronize(dev)
            got = d_results.cpu().numpy().view(srsgpu.PRACH_RESULT_DTYPE)
            C.compare(got[0], dict(cases[0], indications=[]), C.detect(cases[0], C.words_to_complex(cases[0]["words"])),
                      C.new_deviation(), reference=False, fresh_draw=True)

            def launches():
                for _ in range(args.launches):
                    plan.execute(d_input, d_results, torch.cuda.current_stream(dev))

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
            d = C.derive(base["format"], base["ra_scs"], base["n_cs"])
            out = {"case": name, "occasions": count, "workgroups": count * d["nof_sequences"], "ports": base["nof_ports"],
                   "launches_per_round": args.launches}
            for mode, t in times.items():
                out[f"{mode}_us_per_launch"] = {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                                                "max": round(float(np.max(t)), 3)}
            print(json.dumps(out), flush=True)
            plan.close()


if __name__ == "__main__":
    main()
