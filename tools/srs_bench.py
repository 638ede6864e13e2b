#!/usr/bin/env python3
"""Times the SRS estimator launch (srsgpu_srs_estimator_plan_execute) over two plans of 64 resources, one grid each,
with fresh samples: 1 antenna port x 4 rx ports x 1 symbol x 48 PRB with comb 4 (L = 144, 256-point IDFT),
and 4 antenna ports x 4 rx ports x 4 symbols x 272 PRB with comb 2, interleaved (L = 1632, 2048-point IDFT: the largest
resource there is). Each round enqueues --launches executes back to back on one stream between two device events and
synchronises once; the figure is the round's time per launch, median over --rounds. "graph" replays the same launches
captured once. The first resource's result is checked against the float64 restatement before timing. The reference
estimator's time for the same resources on one host core comes from tools/gen_srs_golden.py --time. Run it under
`timeout`; one process. Prints one JSON line per plan."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran-5g_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import srs_cases as C  # noqa: E402
import srsgpu  # noqa: E402


def bench_cases(table):
    """The two resources; tools/gen_srs_golden.py --time runs the reference on the same."""
    return [C.case(table, "bench_small", 48, 0, 4, 1, [0, 1, 2, 3], 1, 0, C.sig(15, 2.3)),
            C.case(table, "bench_wide", 272, 0, 2, 4, [0, 1, 2, 3], 4, 5, C.sig(15, 12.3))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--resources", type=int, default=64)
    args = ap.parse_args()
    ctx = srsgpu.Context(0)
    dev = torch.device("cuda", 0)
    _, table = C.golden()
    for base in bench_cases(table):
        count, prb = args.resources, base["grid_nof_prb"]
        # A few distinct draws, repeated over the grids: the kernel's time does not depend on the samples.
        draws = [C.to_bf16_words(C.make_grid(base, np.random.default_rng([9, i]))) for i in range(4)]
        grids = np.stack([draws[i % len(draws)] for i in range(count)])
        resources = [srsgpu.SrsResource(
            table_row=base["row"], numerology=base["numerology"], nof_antenna_ports=base["nof_antenna_ports"],
            nof_symbols=base["nof_symbols"], start_symbol=base["start_symbol"], comb_size=base["comb_size"],
            comb_offset=base["comb_offset"], cyclic_shift=base["cyclic_shift"], sequence_id=base["sequence_id"],
            bandwidth_index=base["bandwidth_index"], freq_position=base["freq_position"], freq_shift=base["freq_shift"],
            rx_ports=base["rx_ports"], grid_index=i) for i in range(count)]
        plan = srsgpu.SrsEstimatorPlan(ctx, resources, prb, 4, count)
        d_grids = torch.from_numpy(grids.view(np.int32)).to(dev)
        d_results = torch.zeros(srsgpu.SRS_RESULT_DTYPE.itemsize * count, dtype=torch.uint8, device=dev)
        for _ in range(5):
            plan.execute(d_grids, d_results)
        torch.cuda.synchronize(dev)
        got = d_results.cpu().numpy().view(srsgpu.SRS_RESULT_DTYPE)
        want = C.estimate(base, C.words_to_complex(draws[0]))
        bad = C.failures(C.record_as_dict(got[0], base), want, C.tolerances(), check_idx=C.decidable(want))
        assert not bad, (base["name"], bad)

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
        d = C.derive(base)
        out = {"case": base["name"], "resources": count, "L": d["L"], "idft": d["M"], "antenna_ports": base["nof_antenna_ports"],
               "rx_ports": len(base["rx_ports"]), "symbols": base["nof_symbols"], "launches_per_round": args.launches}
        for mode, t in times.items():
            out[f"{mode}_us_per_launch"] = {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                                            "max": round(float(np.max(t)), 3)}
        print(json.dumps(out), flush=True)
        plan.close()


if __name__ == "__main__":
    main()
