"""The timings of profiles/bf16_heads.txt: the four lexical heads at B = 128, L = 128, H = 768, V = 30522, every token unmasked, with logits /
operands of one 16-bit dtype, one process per measurement:

    DHR_HIP_LIB=<libdhr_hip.so> python tools/bf16_heads_timing.py <tag> <float16|bfloat16>     -> one JSON line, milliseconds

lexical and lexical_proj: lexical_reps (forward); lexical_train and lexical_proj_train: lexical_reps(...).backward(G) with every gradient.
Device events, 3 warm-ups, median (and minimum) of 15.  DHR_HIP_LIB (dhr_amd/_lib.py) picks the library, so a build of another commit is timed
with the same script in the same session: alternate the two and take the spread of the repeated runs of one as the margin."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dhr_amd import lexical as LX  # noqa: E402
from dhr_amd import lexical_proj as LP  # noqa: E402
from dhr_amd import lexical_proj_train as LPT  # noqa: E402
from dhr_amd import lexical_train as LT  # noqa: E402

B, L, V, H = 128, 128, 30522, 768
WARM, REPS = 3, 15


def main(tag, dtype):
    dt = getattr(torch, dtype)
    gen = torch.Generator(device="cuda").manual_seed(7)
    hidden = torch.randn((B, L, H), generator=gen, device="cuda").to(dt).requires_grad_(True)
    W = (torch.randn((V, H), generator=gen, device="cuda") * 0.07).to(dt).requires_grad_(True)
    bias = (torch.randn((V,), generator=gen, device="cuda") * 0.1).to(dt).requires_grad_(True)
    w = torch.randn((B, L - 1, 1), generator=gen, device="cuda").requires_grad_(True)
    mask = torch.ones((B, L - 1), dtype=torch.int64, device="cuda")
    G = torch.randn((B, V), generator=gen, device="cuda")
    with torch.no_grad():
        logits = torch.nn.functional.linear(hidden.detach().half(), W.detach().half(), bias.detach().half()).to(dt)
    logits.requires_grad_(True)

    def clear():
        hidden.grad = W.grad = bias.grad = w.grad = logits.grad = None

    heads = {
        "lexical": lambda: LX.lexical_reps(logits[:, 1:], w, mask),
        "lexical_train": lambda: LT.lexical_reps(logits, w, mask, skip_tokens=1).backward(G),
        "lexical_proj": lambda: LP.lexical_reps(hidden[:, 1:], W, bias, w, mask),
        "lexical_proj_train": lambda: LPT.lexical_reps(hidden, W, bias, w, mask, skip_tokens=1).backward(G),
    }
    res = {"tag": tag, "dtype": dtype}
    for name, fn in heads.items():
        times = []
        for it in range(WARM + REPS):
            clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= WARM:
                times.append(e0.elapsed_time(e1))
        res[name] = round(float(np.median(times)), 4)
        res[name + "_min"] = round(float(np.min(times)), 4)
        clear()
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
