"""The fp32 attention family of two builds on the same inputs: outputs compared bit for bit, then timed alternating.
Libraries are given by path: the parent's product and A/B library twice (A and B: two loads of the same build, so the
parent's own spread is known) and the head's.  Shapes a user runs: 10 000 x S = 50, W = 768 (the B/32 vision tower:
mi_op_attention_f32 and mi_op_attention_f32_split roles 0 / 2, and the A/B variants MICLIP_ATTN_F32_V = 4 / 2 / 1),
1 000 x S = 77, W = 512 causal (the text tower) and 200 x S = 257, W = 1024 (L/14, the scalar kernel).
A round's figure is the mean of `reps` back-to-back calls between HIP events, in microseconds; rounds go A H B A H B ...
usage: python scripts/attn_f32_parent_head.py PARENT_A.so PARENT_B.so HEAD.so PARENT_AB_A.so PARENT_AB_B.so HEAD_AB.so [rounds] [reps]"""
import ctypes
import json
import os
import statistics
import sys

import torch


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))   # (after torch: one HIP runtime, as miclip/_native.py)
    P, I32, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    L.mi_op_attention_f32.restype = ctypes.c_int
    L.mi_op_attention_f32.argtypes = [P, P, I32, I32, I32, I32, P]
    L.mi_op_attention_f32_split.restype = ctypes.c_int
    L.mi_op_attention_f32_split.argtypes = [P, P, F, F, P, I32, P, I32, I32, I32, I32, P]
    return L


def main():
    paths = sys.argv[1:7]
    rounds = int(sys.argv[7]) if len(sys.argv) > 7 else 5
    reps = int(sys.argv[8]) if len(sys.argv) > 8 else 10
    prod = dict(zip("AHB", (load(paths[0]), load(paths[2]), load(paths[1]))))
    ab = dict(zip("AHB", (load(paths[3]), load(paths[5]), load(paths[4]))))
    dev = torch.device("cuda:0")
    sp = torch.cuda.current_stream().cuda_stream
    shapes = {"vis": (10000, 50, 768, 0), "text": (1000, 77, 512, 1), "l14": (200, 257, 1024, 0)}
    qkv, rmax = {}, {}
    for name, (B, S, W, causal) in shapes.items():
        g = torch.Generator(device=dev).manual_seed(3 + S)
        qkv[name] = torch.randn(B * S, 3 * W, device=dev, generator=g) * 2
        rmax[name] = qkv[name][:, 2 * W:].abs().amax(dim=1).contiguous()

    # case -> (libraries, shape, MICLIP_ATTN_F32_V or None, split role or None)
    cases = {"vis_f32": (prod, "vis", None, None), "vis_split_role0": (prod, "vis", None, 0),
             "vis_split_role2": (prod, "vis", None, 2), "text_f32": (prod, "text", None, None),
             "l14_f32": (prod, "l14", None, None), "vis_ab_v4": (ab, "vis", "4", None),
             "vis_ab_v2": (ab, "vis", "2", None), "vis_ab_v1": (ab, "vis", "1", None)}

    def call(case, side, out, sc):
        libs, shape, var, role = cases[case]
        B, S, W, causal = shapes[shape]
        if var is None:
            os.environ.pop("MICLIP_ATTN_F32_V", None)
        else:
            os.environ["MICLIP_ATTN_F32_V"] = var
        L = libs[side]
        if role is None:
            rc = L.mi_op_attention_f32(qkv[shape].data_ptr(), out.data_ptr(), B, S, W, causal, sp)
        else:
            rc = L.mi_op_attention_f32_split(qkv[shape].data_ptr(), rmax[shape].data_ptr(), 1.0, 0.0, out.data_ptr(), role,
                                             sc.data_ptr(), B, S, W, causal, sp)
        if rc != 0:
            raise RuntimeError(f"{case} {side}: rc {rc}")

    times = {c: {s: [] for s in "AHB"} for c in cases}
    equal = {}
    for case, (libs, shape, var, role) in cases.items():
        B, S, W, causal = shapes[shape]
        cols = W if role is None else (2 * W if role == 2 else 3 * W)
        dt = torch.float32 if role is None else torch.int16
        outs = {s: torch.zeros(B * S, cols, dtype=dt, device=dev) for s in "AHB"}
        scs = {s: torch.zeros(B * S, device=dev) for s in "AHB"}
        for s in "AHB":   # warm-up and the outputs to compare
            call(case, s, outs[s], scs[s])
        torch.cuda.synchronize()
        view = (lambda t: t.view(torch.int32)) if role is None else (lambda t: t)
        equal[case] = all(torch.equal(view(outs["A"]), view(outs[s])) and
                          torch.equal(scs["A"].view(torch.int32), scs[s].view(torch.int32)) for s in "HB")
        for _ in range(rounds):
            for s in "AHB":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    call(case, s, outs[s], scs[s])
                e1.record()
                torch.cuda.synchronize()
                times[case][s].append(round(e0.elapsed_time(e1) * 1e3 / reps, 2))
        del outs, scs

    print("case | outputs equal | parent A | parent B | parent spread (max-min of the A and B rounds) | head | head - parent | verdict")
    ok = True
    for case in cases:
        t = times[case]
        par = t["A"] + t["B"]
        spread = max(par) - min(par)
        a, h, b = (statistics.median(t[s]) for s in "AHB")
        d = h - statistics.median(par)
        verdict = "within" if abs(d) <= spread else ("FASTER" if d < 0 else "SLOWER")
        ok = ok and equal[case]
        print(f"{case} | {equal[case]} | {a:.1f} | {b:.1f} | {spread:.1f} | {h:.1f} | {d:+.1f} | {verdict}")
    print("# per-round figures")
    for case in cases:
        print(case, json.dumps(times[case]))
    print("RESULT: outputs", "all equal" if ok else "DIFFER")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
