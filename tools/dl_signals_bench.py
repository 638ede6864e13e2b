#!/usr/bin/env python3
"""Times the SS/PBCH block launch (srsgpu_ssb_plan_execute) and the NZP-CSI-RS launch (srsgpu_csi_rs_plan_execute) on the
batches of profiles/dl_signals.md: the fixture's SS/PBCH blocks, each in a 273-PRB x 4-port grid of its own, and 32
slots x one TRS-like row-1 set (symbols 4 and 8) and one row-4 CSI-RS (symbol 13) over 273 PRB. Each round enqueues
--launches executes back to back on one stream between two device events and synchronises once; the figure is the round's
time per launch, median over --rounds. "graph" replays the same launches captured once. The grids are checked against
the fixture and the restatement (tests/ssb_cases.py, tests/csi_rs_cases.py) before timing. The reference's time for the
same work on one host core comes from tools/gen_ssb_golden.py --time and tools/gen_csi_rs_golden.py --time. Prints one
JSON line per batch."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran-5g_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import csi_rs_cases as R  # noqa: E402
import ssb_cases as S  # noqa: E402
import srsgpu  # noqa: E402


def time_launches(args, dev, execute):
    def launches():
        for _ in range(args.launches):
            execute()

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
    return {f"{mode}_us_per_launch": {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                                      "max": round(float(np.max(t)), 3)} for mode, t in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    ctx = srsgpu.Context(0)
    dev = torch.device("cuda", 0)

    # The fixture's SS/PBCH blocks, one grid each.
    golden = list(S.golden_cases())
    blocks = [srsgpu.Ssb(phys_cell_id=c["phys_cell_id"], ssb_idx=c["ssb_idx"], L_max=c["L_max"], pattern_case=c["pattern_case"],
                         common_scs=c["common_scs"], offset_to_pointA=c["offset_to_pointA"],
                         subcarrier_offset=c["subcarrier_offset"], slot_index=c["slot_index"], hrf=c["hrf"], payload=c["payload"],
                         sfn=c["sfn"], ports=c["ports"], pss_amplitude=float(c["pss_amplitude"]), grid_index=i)
              for i, (c, *_) in enumerate(golden)]
    payloads, offsets = srsgpu.ssb_pack_payloads(blocks)
    plan = srsgpu.SsbPlan(ctx, blocks, 273, 4, len(blocks), offsets)
    d_payloads = torch.from_numpy(payloads).to(dev)
    d_grids = torch.zeros(len(blocks) * 4 * 14 * 12 * 273, dtype=torch.int32, device=dev)
    for _ in range(5):
        plan.execute(d_payloads, d_grids)
    torch.cuda.synchronize(dev)
    got = d_grids.cpu().numpy().view(np.uint32).reshape(len(blocks), 4, 14, 12 * 273)
    for i, (_cfg, _l, _k, _enc, rows) in enumerate(golden):
        want = np.zeros((4, 14, 12 * 273), np.uint32)
        S.apply_rows(want, rows)
        assert np.array_equal(got[i], want), i
    out = {"plan": "ssb", "blocks": len(blocks), "grid_words_written": int(sum(r[4].shape[0] for r in golden)),
           "launches_per_round": args.launches}
    out.update(time_launches(args, dev, lambda: plan.execute(d_payloads, d_grids, torch.cuda.current_stream(dev))))
    print(json.dumps(out), flush=True)
    plan.close()
    del d_grids

    # 32 slots x (two row-1 symbols, one row 4) over 273 PRB.
    cases = R.bench_cases(np.random.default_rng(7))
    signals = [srsgpu.CsiRs(slot_index=c["n_slot"], start_rb=c["start_rb"], nof_rb=c["nof_rb"], row=c["row"], k_ref=[c["k_ref"]],
                            symbol_l0=c["symbol_l0"], cdm=c["cdm"], freq_density=c["freq_density"],
                            scrambling_id=c["scrambling_id"], amplitude=float(c["amplitude"]), weights=c["weights"],
                            symbol_l1=c["symbol_l1"], cp=c["cp"], grid_index=c["grid_index"]) for c in cases]
    plan = srsgpu.CsiRsPlan(ctx, signals, 273, 4, 32)
    d_grids = torch.zeros(32 * 4 * 14 * 12 * 273, dtype=torch.int32, device=dev)
    for _ in range(5):
        plan.execute(d_grids)
    torch.cuda.synchronize(dev)
    got = d_grids.cpu().numpy().view(np.uint32).reshape(32, 4, 14, 12 * 273)
    words = 0
    for g in (0, 31):
        want = np.zeros((4, 14, 12 * 273), np.uint32)
        for c in cases:
            if c["grid_index"] == g:
                R.apply_rows(want, R.process(c))
        assert np.array_equal(got[g], want), g
    for c in cases:
        words += R.seq_len(c) * len(R.groups(c)) * R.ROW_PORTS[c["row"]]
    out = {"plan": "csi_rs", "signals": len(signals), "slots": 32, "grid_words_written": int(words),
           "launches_per_round": args.launches}
    out.update(time_launches(args, dev, lambda: plan.execute(d_grids, torch.cuda.current_stream(dev))))
    print(json.dumps(out), flush=True)
    plan.close()


if __name__ == "__main__":
    main()
