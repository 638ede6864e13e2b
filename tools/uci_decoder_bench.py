#!/usr/bin/env python3
"""Times the short-block UCI decoder launch (srsgpu_uci_decoder_plan_execute) on the slot-shaped batches of
profiles/uci_decoder.md: 64 UEs x (HARQ-ACK A = 4, E = 96; CSI Part 1 A = 11, E = 240), one slot and 16 slots per plan.
Each round enqueues --launches executes back to back on one stream between two device events and synchronises once;
the figure is the round's time per launch, median over --rounds. The outputs are checked against the restatement
(tests/uci_cases.py) before timing. The reference detector's time for the same fields on one host core comes from
tools/gen_uci_golden.py --time. Prints one JSON line per batch."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "srsran-5g_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import srsgpu  # noqa: E402
import uci_cases as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    ctx = srsgpu.Context(0)
    dev = torch.device("cuda", 0)
    for slots in (1, 16):
        fields = C.slot_batch_fields(np.random.default_rng(5), nof_slots=slots)
        # HARQ-ACK fields in source 0, CSI Part 1 fields in source 1, as the demultiplexer leaves them.
        offs, cfgs = [0, 0], []
        for llrs, a, qm, _ in fields:
            s = 0 if a == 4 else 1
            cfgs.append((a, qm, s, llrs.size, offs[s]))
            offs[s] += llrs.size
        d_src = [torch.from_numpy(np.concatenate([f[0] for f in fields if (f[1] == 4) == (s == 0)])).to(dev)
                 for s in (0, 1)]
        plan = srsgpu.UciDecoderPlan(ctx, cfgs)
        d_msgs = torch.zeros(len(fields), dtype=torch.int16, device=dev)
        d_status = torch.zeros(len(fields), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        for _ in range(20):
            plan.execute(d_src[0], d_src[1], None, d_msgs, d_status, stream)
        torch.cuda.synchronize(dev)
        msgs, status = d_msgs.cpu().numpy().view(np.uint16), d_status.cpu().numpy()
        for f, m, v in zip(fields, msgs, status):
            bits, valid, _ = C.detect(f[0], f[1], f[2])
            assert int(m) == sum(int(b) << j for j, b in enumerate(bits)) and bool(v) == valid
        def launches():
            for _ in range(args.launches):
                plan.execute(d_src[0], d_src[1], None, d_msgs, d_status, torch.cuda.current_stream(dev))

        # The same launches captured once and replayed: the device's time per launch without the host's enqueue cost.
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
        out = {"batch": f"{slots} slot(s) x 64 UEs x (A=4 E=96, A=11 E=240)", "fields": len(fields),
               "llr_bytes": int(sum(f[0].size for f in fields)), "launches_per_round": args.launches}
        for mode, t in times.items():
            out[f"{mode}_us_per_launch"] = {"median": round(float(np.median(t)), 3), "min": round(float(np.min(t)), 3),
                                            "max": round(float(np.max(t)), 3)}
        print(json.dumps(out), flush=True)
        plan.close()


if __name__ == "__main__":
    main()
