"""Writes tests/golden/lz4_foreign_frames.npz: a few inputs and the frames LIBLZ4 makes of them (LZ4F_compressFrame, 64 KiB
independent blocks, no checksums - the form the library reads), so that a machine without liblz4 can still feed the decoders
frames that another encoder wrote.  Run on a machine with liblz4:  python tests/golden/make_lz4_foreign_frames.py
Layout: `inputs` / `frames` are the byte strings back to back, `input_off` / `frame_off` their n + 1 starts, `names` the labels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lz4_cases as Z  # noqa: E402

CASES = [("one byte", 65536), ("period 2", 65549), ("period 3", 131072 + 5), ("period 16", 65537), ("period 64", 13), ("period 64", 12),
         ("random", 0), ("random", 1), ("random", 65), ("random", 4096)]


def main():
    assert Z.liblz4() is not None, "this script needs liblz4"
    items = [("%s x %d" % c, Z.pattern(*c)) for c in CASES]
    mixed = Z.mixed_inputs()
    small = [i for i, d in enumerate(mixed) if len(d) < 3000][:3]
    mid = [i for i, d in enumerate(mixed) if 30000 < len(d) < 70000][:1]
    items += [("mixed %d" % i, mixed[i]) for i in small + mid]
    frames = [Z.liblz4_frame(d, block_size_id=4, independent=True) for _, d in items]
    for (_, d), f in zip(items, frames):
        assert Z.walk_frames(f)[0][0] == d if d else f == Z.HEADER + Z.ENDMARK
    cat = lambda xs: np.frombuffer(b"".join(xs), dtype=np.uint8)
    offs = lambda xs: np.cumsum([0] + [len(x) for x in xs]).astype(np.uint64)
    path = os.path.join(HERE, "lz4_foreign_frames.npz")
    np.savez_compressed(path, names=np.array([n for n, _ in items]), inputs=cat([d for _, d in items]), input_off=offs([d for _, d in items]),
                        frames=cat(frames), frame_off=offs(frames))
    size = os.path.getsize(path)
    assert size < 256 << 10, size
    print("%s: %d cases, %d bytes" % (path, len(items), size))


if __name__ == "__main__":
    main()
