#!/usr/bin/env python3
"""ucfvit_seg_counts (csrc/seg_metric.hip: argmax label map + Dice counts in one pass) at the UNETR workload's size, B = 2, 512 x 512 x 128,
n = 4 classes, in both layouts (N C D H W; channels-last, the HIP decoder's own: dense rows ld = 4, and padded rows ld = 8) and both
dtypes, against the torch statement of the same thing (argmax, one_hot of prediction and label, their product, sums) in the same process,
and against the bytes the pass must move: n logits + an 8-byte label + a 1-byte prediction per voxel (a padded row is fetched whole: the
`fetched` figures count ld logits).  Bandwidth fractions are of the 6.29 TB/s a float4 copy reaches on an MI355X (8.0 TB/s is the HBM3E
specification).

  python tools/seg_metric_bench.py [reps=200] [torch_reps=5]

Times are HIP-event times over `reps` back-to-back calls after a warm-up call (the torch statement: `torch_reps`); the results of the two
are compared bit for bit before anything is timed.  One JSON line per case on stdout."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ucf-vit_amd"))
from UCF_VIT._hip import ops  # noqa: E402

DEV = "cuda"
B, VOL, N = 2, (512, 512, 128), 4
STREAM_TBPS, SPEC_TBPS = 6.29, 8.0


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def torch_statement(logits, lab):
    pred = torch.argmax(logits.float(), dim=1)
    oh_p = torch.nn.functional.one_hot(pred, N)
    oh_y = torch.nn.functional.one_hot(lab, N)
    s = lambda t: t.reshape(B, -1, N).sum(dim=1)
    return pred, torch.stack([s(oh_p * oh_y), s(oh_p), s(oh_y)], dim=1)


def main(reps, torch_reps):
    g = torch.Generator(device=DEV).manual_seed(0)
    S = VOL[0] * VOL[1] * VOL[2]
    lab = torch.randint(0, N, (B, *VOL), generator=g, device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        for layout, ld in (("ncdhw", 0), ("channels-last", N), ("channels-last", 8)):
            if ld:
                buf = torch.randn((B, *VOL, ld), generator=g, device=DEV).to(dtype)
                logits = buf[..., :N].permute(0, 4, 1, 2, 3)
            else:
                logits = torch.randn((B, N, *VOL), generator=g, device=DEV).to(dtype)
            route = ops.seg_counts_route(logits, lab)
            pred, counts = ops.seg_counts(logits, lab)
            want_pred, want_counts = torch_statement(logits, lab)
            if not (torch.equal(pred.long(), want_pred) and torch.equal(counts, want_counts)):
                raise SystemExit(f"seg_counts differs from the torch statement: {dtype} {layout} ld {ld}")
            del want_pred, want_counts, pred, counts
            t_k = _timed(lambda: ops.seg_counts(logits, lab), reps)
            t_np = _timed(lambda: ops.seg_counts(logits, lab, want_pred=False), reps)
            t_t = _timed(lambda: torch_statement(logits, lab), torch_reps)
            es = logits.element_size()
            must = B * S * (N * es + 8 + 1)
            fetched = B * S * ((ld or N) * es + 8 + 1)
            print(json.dumps({"dtype": str(dtype).split(".")[1], "layout": layout, "ld": ld or None, "route": route, "seg_counts_ms": round(t_k, 4),
                              "seg_counts_no_pred_ms": round(t_np, 4), "torch_ms": round(t_t, 3), "speedup": round(t_t / t_k, 1),
                              "must_move_bytes": must, "must_move_TBps": round(must / t_k / 1e9, 3),
                              "frac_of_stream_6.29": round(must / t_k / 1e9 / STREAM_TBPS, 3), "frac_of_spec_8.0": round(must / t_k / 1e9 / SPEC_TBPS, 3),
                              "fetched_bytes": fetched, "fetched_TBps": round(fetched / t_k / 1e9, 3)}), flush=True)
            del logits


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
