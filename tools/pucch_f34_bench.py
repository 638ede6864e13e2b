#!/usr/bin/env python3
"""Times the PUCCH Format 3 / 4 launches over three plans: the fixture's PDUs (tests/golden/pucch_f34.npz, one grid
each), a 32-slot batch of 8 PDUs per slot (tests/pucch_f34_cases.py bench_batch_cases: 52 PRBs x 4 ports, Format 3 of
1..4 PRB and Format 4, 4..14 symbols, payloads of 4..40 bits) and the largest PDU alone (Format 3, 16 PRB, 14 symbols,
4 ports: one workgroup, the worst case of the direct inverse DFT). "front_end" is srsgpu_pucch_f34_plan_execute alone
(one launch); "process" adds the short-block and the polar UCI decoder launches on the same stream (three launches,
PucchF34Batch.launch). Each round enqueues --launches repetitions back to back on one stream between two device events
and synchronises once; the figure is the round's time per repetition, median over --rounds. "graph" replays the same
repetitions captured once. Before timing, the LLRs of about 40 PDUs spread over the plan are checked against the
float64 restatement (equal or one step apart). The reference path's time for the same PDUs on one host core comes from
tools/gen_pucch_f34_golden.py --time. Run it under `timeout`; one process. Prints one JSON line per plan."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran-5g_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch  # noqa: E402

import pucch_f34_cases as C  # noqa: E402
import srsgpu  # noqa: E402


def to_pdu(cfg, grid_index):
    common = dict(slot_index=cfg["slot_index"], starting_prb=cfg["starting_prb"], start_symbol_index=cfg["start_symbol"],
                  nof_symbols=cfg["nof_symbols"], rnti=cfg["rnti"], n_id_scrambling=cfg["n_id_scrambling"],
                  n_id_hopping=cfg["n_id_hopping"], nof_csi_part1=cfg["nof_uci_bits"], ports=cfg["ports"],
                  second_hop_prb=None if cfg["second_hop_prb"] == C.NO_HOP else cfg["second_hop_prb"],
                  additional_dmrs=bool(cfg["additional_dmrs"]), pi2_bpsk=bool(cfg["pi2_bpsk"]), numerology=cfg["numerology"],
                  cp_extended=cfg["cp_extended"], grid_index=grid_index)
    if cfg["format"] == 4:
        return srsgpu.PucchF4(occ_length=cfg["occ_length"], occ_index=cfg["occ_index"], **common)
    return srsgpu.PucchF3(nof_prb=cfg["nof_prb"], **common)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    ctx = srsgpu.Context(0)
    dev = torch.device("cuda", 0)
    fixture = [(c["cfg"], c["words"], i) for i, c in enumerate(C.golden())]
    plans = (("fixture", fixture, max(cfg["grid_nof_prb"] for cfg, *_ in fixture), len(fixture)),
             ("32_slots_x_8", C.bench_batch_cases(np.random.default_rng(C.BENCH_SEED)), 52, 32),
             ("f3_16prb_14sym_4ports", [C.worst_case(np.random.default_rng(C.BENCH_SEED))], 52, 1))
    for name, placed, grid_prb, nof_grids in plans:
        grids = C.place(placed, grid_prb, 4, nof_grids)
        batch = srsgpu.PucchF34Batch(ctx, [to_pdu(cfg, g) for cfg, _, g in placed], grid_prb, 4, nof_grids)
        d_grids = torch.from_numpy(grids.view(np.int32)).to(dev)
        for _ in range(5):
            batch.launch(d_grids)
        torch.cuda.synchronize(dev)
        llrs, _ = batch.raw()
        zgrids = C.words_to_complex(grids)
        for (cfg, _, g), o in list(zip(placed, batch.front.llr_offsets))[:: max(1, len(placed) // 40)]:
            want = C.restate(cfg, zgrids[g])["llrs"]
            assert C.llr_diff(llrs[o: o + want.size], want)[1] <= 1, cfg

        def front_end():
            for _ in range(args.launches):
                batch.front.execute(d_grids, batch.d_llrs, batch.d_results)  # on the current stream: the capture's

        def process():
            for _ in range(args.launches):
                batch.launch(d_grids)

        out = {"plan": name, "pdus": len(placed), "grids": nof_grids, "llrs": batch.front.nof_llrs,
               "short_block_pdus": len(batch.short_ids), "polar_pdus": len(batch.polar_ids),
               "launches_per_round": args.launches}
        for what, body in (("front_end", front_end), ("process", process)):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                body()
            graph.replay()
            torch.cuda.synchronize(dev)
            times = {"eager": [], "graph": []}
            for _ in range(args.rounds):
                for mode, run in (("eager", body), ("graph", graph.replay)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    e1.synchronize()
                    times[mode].append(e0.elapsed_time(e1) * 1e3 / args.launches)
            for mode, t in times.items():
                out[f"{what}_{mode}_us"] = {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                                           "max": round(float(np.max(t)), 3)}
            del graph
        print(json.dumps(out), flush=True)
        batch.close()


if __name__ == "__main__":
    main()
