"""Workload for a kernel trace of the Aggretriever training ops (profiles/aggretriever_train.txt):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/aggretriever_trace.py
The shapes of the reference's Aggretriever recipe (24 queries x 8 passages per device, q_max_len 32, p_max_len 150, agg_dim 640, BERT's 30522
ids), fp16 term weights; 3 forward + backward calls per shape of the no-MLM chain aggregate(term_weight_reps(...)) and of aggregate alone on
dense fp32 reps (what follows the MLM head).
    python tools/aggretriever_trace.py --time
prints instead the step times (device events around windows of 100 steps after a warm-up of 5, three repeats) and the peak memory of one step, this
library and the eager composition of the reference's ops alternating in one process."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dhr_amd import aggretriever_train as AT  # noqa: E402
from dhr_amd.lexical import cal_remove_dim  # noqa: E402

V, DIMS = 30522, 640
SHAPES = (("queries", 24, 32), ("passages", 192, 150))


def eager_aggregate(reps, dims, full):
    """tevatron/Aggretriever/utils.py:22-44"""
    B = reps.shape[0]
    if full:
        remove = cal_remove_dim(dims * 2)
        if remove >= 0:
            reps = reps[:, remove:].view(B, -1, dims * 2)
        else:
            reps = torch.nn.functional.pad(reps, (0, -remove), "constant", 0).view(B, -1, dims * 2)
        tok, _ = reps.max(1)
        pos, neg = tok[:, 0:2 * dims:2], tok[:, 1:2 * dims:2]
        return pos * (pos > neg) - neg * (pos <= neg)
    return reps[:, cal_remove_dim(dims):].view(B, -1, dims).max(1)[0]


def eager_head(ids, w):
    """tevatron/Aggretriever/modeling.py:282-284"""
    reps = torch.zeros(ids.shape[0], ids.shape[1], V, dtype=w.dtype, device=w.device)
    return torch.scatter(reps, dim=-1, index=ids[:, 1:, None], src=w).max(-2).values


def inputs(B, L, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ids = torch.randint(1000, V, (B, L), generator=gen, device="cuda")
    ids[:, 3 * L // 4:] = 0                                                       # a quarter of every row is padding
    w = torch.randn((B, L - 1, 1), generator=gen, device="cuda").half().requires_grad_(True)
    dense = torch.randn((B, V), generator=gen, device="cuda").requires_grad_(True)
    return ids, w, dense, torch.randn((B, DIMS), generator=gen, device="cuda")


def cases(ids, w, dense, G):
    """name -> (this library's step, the eager step)"""
    def chain(head, agg):
        def step():
            w.grad = None
            out = agg(head(ids, w), DIMS, True)
            out.backward(G.to(out.dtype))
        return step

    def alone(agg):
        def step():
            dense.grad = None
            agg(dense, DIMS, True).backward(G)
        return step
    return {"no-MLM chain, fp16 weights": (chain(AT.term_weight_reps, AT.aggregate), chain(eager_head, eager_aggregate)),
            "aggregate alone, dense fp32 reps": (alone(AT.aggregate), alone(eager_aggregate))}


def window(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def peak(step):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    timed = "--time" in sys.argv
    for name, B, L in SHAPES:
        ids, w, dense, G = inputs(B, L, B)
        for case, (fused, eager) in cases(ids, w, dense, G).items():
            if not timed:
                for _ in range(3):
                    fused()
                torch.cuda.synchronize()
                print("%s %d x %d: %s done" % (name, B, L, case))
                continue
            times = {"fused": [], "eager": []}
            for _ in range(3):
                for side, step in (("fused", fused), ("eager", eager)):
                    window(step, 5)
                    times[side].append(window(step, 100))
            mem = {}
            for side, step in (("fused", fused), ("eager", eager)):
                w.grad = dense.grad = None                                        # the returned gradient is inside the figure
                mem[side] = peak(step)
            f, e = sorted(times["fused"])[1], sorted(times["eager"])[1]
            print("%s %d x %d, %s: fused %s ms, eager torch %s ms, eager / fused %.1fx; peak memory of a step fused %.1f MB, eager %.1f MB" % (
                name, B, L, case, " / ".join("%.3f" % t for t in times["fused"]), " / ".join("%.3f" % t for t in times["eager"]), e / f,
                mem["fused"] / 1e6, mem["eager"] / 1e6), flush=True)
        del ids, w, dense, G
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
