"""The JPEG decode of two builds on the same input: outputs compared bit for bit, then timed alternating (the method
of scripts/attn_f32_parent_head.py).  Libraries are given by path: the parent's product and A/B library twice (A and B:
two copies of the same build, so the box's own spread is known) and the head's.  Input: the 16 reference frames of
tests/golden/ref_frames (1280 x 720, 4:2:0) tiled to 2048 frames, the ingest pipeline's launch size.
Cases: mi_jpeg_decode_transform (n = 224, bf16) and mi_jpeg_decode on the product libraries (the chunked entropy
kernels, the IDCT, the fused transform / the colour kernel), and mi_jpeg_decode with MICLIP_JPEG_SERIAL=1 on the A/B
libraries (jpeg_entropy_kernel<true>, 256 frames: a lane per frame).
A round's figure is the mean of `reps` back-to-back calls between HIP events, in milliseconds; rounds go A H B A H B ...
Pass: every head round lies inside [min, max] of the parent's rounds (A and B) widened by the largest |A - B| of any
round -- A and B are the same code, so that gap is the box's noise.
usage: python scripts/jpeg_parent_head.py PARENT_A.so PARENT_B.so HEAD.so PARENT_AB_A.so PARENT_AB_B.so HEAD_AB.so [rounds] [reps]"""
import ctypes
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "event-retrival-in-video-learning-transferable-visual-model-from-supervised-natural-language_amd"))


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))   # (after torch: one HIP runtime, as miclip/_native.py)
    P, I32, I64, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    L.mi_jpeg_workspace_bytes.restype = SZ
    L.mi_jpeg_workspace_bytes.argtypes = [P, I32, I64]
    L.mi_jpeg_decode.restype = ctypes.c_int
    L.mi_jpeg_decode.argtypes = [P, I64, P, P, P, P, I32, P, P, I32, P, P, SZ, P]
    L.mi_jpeg_decode_transform.restype = ctypes.c_int
    L.mi_jpeg_decode_transform.argtypes = [P, I64, P, P, P, P, I32, P, P, I32, I32, ctypes.c_int, P, ctypes.c_int, P, SZ, P]
    return L


class Batch:
    """mi_jpeg_decode's arguments for B frames (the reference frames repeated), on the device."""

    def __init__(self, raw, B, dev):
        from miclip import jpeg
        bufs = [raw[i % len(raw)] for i in range(B)]
        heads = [jpeg.parse(b) for b in bufs]
        segl = [((h.scan_start, len(b)),) for h, b in zip(heads, bufs)]
        self.geom, huff, hidx, qt, offs, ends, starts, self.nsets = jpeg.launch_args(
            bufs, heads, list(range(B)), segl, jpeg._geom_key(heads[0]))
        data = b"".join(b[h.scan_start:] for h, b in zip(heads, bufs))
        self.B, self.total = B, len(data)
        self.W, self.H = int(self.geom[0]), int(self.geom[1])
        self.data = torch.frombuffer(bytearray(data + b"\xff\xd9" * 16), dtype=torch.uint8).to(dev)
        self.huff = torch.from_numpy(huff.view(np.uint8).reshape(-1)).to(dev)
        self.hidx = torch.from_numpy(np.ascontiguousarray(hidx)).to(dev)
        self.qt = torch.from_numpy(np.ascontiguousarray(qt)).to(dev)
        self.off, self.end = torch.from_numpy(offs).to(dev), torch.from_numpy(ends).to(dev)

    def args(self):
        return (self.data.data_ptr(), self.total, self.off.data_ptr(), self.end.data_ptr(), self.huff.data_ptr(),
                self.hidx.data_ptr(), self.nsets, self.qt.data_ptr(), self.geom.ctypes.data, self.B)


def main():
    paths = sys.argv[1:7]
    rounds = int(sys.argv[7]) if len(sys.argv) > 7 else 5
    reps = int(sys.argv[8]) if len(sys.argv) > 8 else 3
    prod = dict(zip("AHB", (load(paths[0]), load(paths[2]), load(paths[1]))))
    ab = dict(zip("AHB", (load(paths[3]), load(paths[5]), load(paths[4]))))
    dev = torch.device("cuda:0")
    sp = torch.cuda.current_stream().cuda_stream
    raw = [open(f, "rb").read() for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_frames", "*.jpg")))]
    assert len(raw) == 16
    big, small = Batch(raw, 2048, dev), Batch(raw, 256, dev)

    # case -> (libraries, batch, fused transform?, MICLIP_JPEG_SERIAL, reps)
    cases = {"decode_transform_224_bf16": (prod, big, True, None, reps), "decode_rgb": (prod, big, False, None, reps),
             "decode_rgb_serial_ab": (ab, small, False, "1", 1)}
    times = {c: {s: [] for s in "AHB"} for c in cases}
    equal = {}
    for case, (libs, bt, fused, serial, nrep) in cases.items():
        if serial is None:
            os.environ.pop("MICLIP_JPEG_SERIAL", None)
        else:
            os.environ["MICLIP_JPEG_SERIAL"] = serial
        need = {s: libs[s].mi_jpeg_workspace_bytes(bt.geom.ctypes.data, bt.B, bt.total) for s in "AHB"}
        assert need["A"] == need["H"] == need["B"], need
        ws = torch.empty(need["A"], dtype=torch.uint8, device=dev)
        shape = (bt.B, 3, 224, 224) if fused else (bt.B, bt.H, bt.W, 3)
        outs = {s: torch.zeros(shape, dtype=torch.bfloat16 if fused else torch.uint8, device=dev) for s in "AHB"}

        def call(s):
            L = libs[s]
            if fused:
                rc = L.mi_jpeg_decode_transform(*bt.args(), 224, 0, outs[s].data_ptr(), 1, ws.data_ptr(), need["A"], sp)
            else:
                rc = L.mi_jpeg_decode(*bt.args(), outs[s].data_ptr(), ws.data_ptr(), need["A"], sp)
            if rc != 0:
                raise RuntimeError(f"{case} {s}: rc {rc}")

        for s in "AHB":   # warm-up and the outputs to compare
            call(s)
        torch.cuda.synchronize()
        view = (lambda t: t.view(torch.int16)) if fused else (lambda t: t)
        equal[case] = all(torch.equal(view(outs["A"]), view(outs[s])) for s in "HB") and bool(outs["A"].any())
        for _ in range(rounds):
            for s in "AHB":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(nrep):
                    call(s)
                e1.record()
                torch.cuda.synchronize()
                times[case][s].append(round(e0.elapsed_time(e1) / nrep, 3))
        del outs, ws
        torch.cuda.empty_cache()

    print("case | outputs equal | parent rounds min..max | largest A-B gap of a round | head rounds min..max | verdict")
    ok = True
    for case in cases:
        t = times[case]
        par = t["A"] + t["B"]
        gap = max(abs(a - b) for a, b in zip(t["A"], t["B"]))
        lo, hi = min(par) - gap, max(par) + gap
        inside = all(lo <= h <= hi for h in t["H"])
        verdict = "within" if inside else ("FASTER" if max(t["H"]) < lo or min(t["H"]) < lo and max(t["H"]) <= hi else "SLOWER")
        ok = ok and equal[case] and verdict != "SLOWER"
        print(f"{case} | {equal[case]} | {min(par):.3f}..{max(par):.3f} ms | {gap:.3f} ms | {min(t['H']):.3f}..{max(t['H']):.3f} ms"
              f" | {verdict}")
    print("# per-round figures (ms)")
    for case in cases:
        print(case, json.dumps(times[case]))
    print("RESULT:", "outputs all equal, head inside the parent's range" if ok else "FAILED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
