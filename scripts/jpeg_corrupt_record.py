"""Recorded decodes of damaged JPEG scans: tests/golden/jpeg_corrupt_digests.json.

The serial (lane-per-frame) and the chunked entropy kernels share one symbol step, so comparing
them with each other no longer checks what that step does with damaged data: a run past
coefficient 63, a code with no match, a marker in the middle of the scan, the zero feed after a
truncation.  This script records what the serial kernel gave when the two steps were still written
out separately; tests/test_gpu_jpeg.py::test_corrupt_streams_match_record holds both paths to it.

Inputs: each of the 16 frames of tests/golden/ref_frames (1280 x 720, 225 chunks per scan) in two
damaged variants, variants() below -- every position follows from the buffer's length and its scan
start, nothing is random.  Recorded: the sha256 of each input buffer and of each decoded RGB frame
(A/B library, MICLIP_JPEG_SERIAL=1).  The chunked default path must give the same frames at the
recording build too; the script refuses to write a record when it does not.

usage: python scripts/jpeg_corrupt_record.py [OUT.json]     (needs a GPU and the A/B library)"""
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "event-retrival-in-video-learning-transferable-visual-model-from-supervised-natural-language_amd")
RECORD = os.path.join(ROOT, "tests", "golden", "jpeg_corrupt_digests.json")


def frame_files():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_frames", "*.jpg")))


def variants(buf, i, scan_start, nframes=16):
    """(corrupted, truncated) variants of frame i's file; both keep the headers and end in an EOI,
    so both stay on the device path.  With n = the entropy-coded bytes before the final EOI:
      corrupted  6 + i single bytes XORed (spread over the scan: wrong codes, wrong extra bits);
                 8 + 2 (i % 5) bytes from n (3 + i) / 24 on overwritten with FF -- stuffed (FF 00
                 pairs: a stretch of 1 bits, codes longer than any in the table) except in every
                 fourth frame, where the bare FF FF ends the data as a marker does;
                 FF D3 written at n (13 + i % 7) / 24 (a marker mid-scan: zeros from there on);
      truncated  cut at n (i + 1) / (nframes + 2), then the EOI."""
    lo, hi = scan_start, len(buf) - 2
    n = hi - lo
    b = bytearray(buf)
    for j in range(6 + i):
        p = lo + (n * (2 * j + 1)) // (2 * (6 + i)) + (7 * i + 3 * j) % 11
        b[min(p, hi - 1)] ^= 1 + (37 * j + 11 * i) % 255
    p = lo + n * (3 + i) // 24
    ln = 8 + 2 * (i % 5)
    b[p:p + ln] = b"\xff" * ln if i % 4 == 3 else b"\xff\x00" * (ln // 2)
    p = lo + n * (13 + i % 7) // 24
    b[p:p + 2] = b"\xff\xd3"
    cut = lo + n * (i + 1) // (nframes + 2)
    return bytes(b), buf[:cut] + b"\xff\xd9"


def inputs():
    """The 32 buffers, frame order, (corrupted, truncated) per frame."""
    sys.path.insert(0, PKG)
    from miclip import jpeg
    files = frame_files()
    assert len(files) == 16
    out = []
    for i, f in enumerate(files):
        with open(f, "rb") as fh:
            buf = fh.read()
        out += variants(buf, i, jpeg.parse(buf).scan_start)
    return out


def sha(x):
    return hashlib.sha256(x).hexdigest()


def decode_digests(bufs, serial):
    """sha256 of every decoded frame: the product library's default (chunked) path, or the A/B
    library's serial kernel."""
    from miclip import _native, jpeg
    saved = _native.lib, os.environ.get("MICLIP_JPEG_SERIAL")
    try:
        if serial:
            _native.lib = _native.lib_ab
            os.environ["MICLIP_JPEG_SERIAL"] = "1"
        got = jpeg.decode_batch(bufs, "cuda")
    finally:
        _native.lib = saved[0]
        if serial:
            os.environ.pop("MICLIP_JPEG_SERIAL")
            if saved[1] is not None:
                os.environ["MICLIP_JPEG_SERIAL"] = saved[1]
    assert all(g is not None for g in got)
    return [sha(g.cpu().numpy().tobytes()) for g in got]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else RECORD
    bufs = inputs()
    from miclip import jpeg
    assert all(jpeg.parse(b).supported for b in bufs)
    ser = decode_digests(bufs, serial=True)
    chk = decode_digests(bufs, serial=False)
    bad = [i for i in range(len(bufs)) if ser[i] != chk[i]]
    if bad:
        print(f"chunked decode differs from the serial kernel on buffers {bad}: a bug, nothing recorded")
        return 1
    rec = {"inputs": [sha(b) for b in bufs], "rgb": ser}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"recorded {len(bufs)} buffers ({len(set(ser))} distinct frames) -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
