#!/usr/bin/env python3
"""Times the PDCCH launch (srsgpu_pdcch_plan_execute) on the batches of profiles/pdcch.md: 32, 256 and 2048 DCIs of
mixed aggregation levels (1, 2, 4, 8, 16, 4, 2, 8 per slot: 45 CCEs of an interleaved two-symbol CORESET over 270 PRBs),
eight DCIs per 273-PRB x 4-port grid, four ports each. Each round enqueues --launches executes back to back on one
stream between two device events and synchronises once; the figure is the round's time per launch, median over
--rounds. "graph" replays the same launches captured once. The grids are checked against the restatement
(tests/pdcch_cases.py) before timing. The reference processor's time for the same DCIs on one host core comes from
tools/gen_pdcch_golden.py --time. Prints one JSON line per batch."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran-5g_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import pdcch_cases as C  # noqa: E402
import srsgpu  # noqa: E402


def to_dci(cfg, payload):
    return srsgpu.Pdcch(
        bwp_size_rb=cfg["bwp_size_rb"], bwp_start_rb=cfg["bwp_start_rb"], start_symbol=cfg["start_symbol"],
        duration=cfg["duration"], frequency_resources=cfg["frequency_resources"], mapping=cfg["mapping"],
        slot_index=cfg["n_slot"], rnti=cfg["rnti"], n_id_pdcch_dmrs=cfg["n_id_dmrs"], n_id_pdcch_data=cfg["n_id_data"],
        n_rnti=cfg["n_rnti"], cce_index=cfg["cce_index"], aggregation_level=cfg["aggregation_level"], payload=payload,
        weights=cfg["weights"], reg_bundle_size=cfg["reg_bundle_size"], interleaver_size=cfg["interleaver_size"],
        shift_index=cfg["shift_index"], data_scaling=float(cfg["data_scaling"]),
        dmrs_amplitude=float(cfg["dmrs_amplitude"]), grid_index=cfg["grid_index"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--check", type=int, default=2, help="grids per batch checked against the restatement")
    args = ap.parse_args()
    ctx = srsgpu.Context(0)
    dev = torch.device("cuda", 0)
    for nof_dcis in (32, 256, 2048):
        cases = C.bench_cases(np.random.default_rng(7), nof_dcis)
        dcis = [to_dci(c, p) for c, p in cases]
        nof_grids = nof_dcis // 8
        payloads, offsets = srsgpu.pdcch_pack_payloads(dcis)
        plan = srsgpu.PdcchPlan(ctx, dcis, 273, 4, nof_grids, offsets)
        d_payloads = torch.from_numpy(payloads).to(dev)
        d_grids = torch.zeros(nof_grids * 4 * 14 * 12 * 273, dtype=torch.int32, device=dev)
        for _ in range(5):
            plan.execute(d_payloads, d_grids)
        torch.cuda.synchronize(dev)
        got = d_grids.cpu().numpy().view(np.uint32).reshape(nof_grids, 4, 14, 12 * 273)
        for g in sorted({0, nof_grids - 1})[: args.check]:
            want = np.zeros((4, 14, 12 * 273), np.uint32)
            for cfg, payload in cases[8 * g: 8 * g + 8]:
                C.apply_rows(want, C.process(cfg, payload)[2])
            assert np.array_equal(got[g], want), g

        def launches():
            for _ in range(args.launches):
                plan.execute(d_payloads, d_grids, torch.cuda.current_stream(dev))

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
        out = {"dcis": nof_dcis, "grids": nof_grids, "grid_words_written": int(sum(72 * c["aggregation_level"] * 4 for c, _ in cases)),
               "launches_per_round": args.launches}
        for mode, t in times.items():
            out[f"{mode}_us_per_launch"] = {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                                            "max": round(float(np.max(t)), 3)}
        print(json.dumps(out), flush=True)
        plan.close()


if __name__ == "__main__":
    main()
