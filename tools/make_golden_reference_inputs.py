"""Fixtures that let the ingestion tests run without the reference checkout.

    python tools/make_golden_reference_inputs.py REFERENCE_DIR

tests/golden/reference_scene_<name>.npz (glassSphere, ring, veach): what the reference's own
input/scenes/<name>.json gives when it is loaded from its checkout -- the blob's counts, every
render session's RenderParams, and the oracle's 40x24x2spp framebuffer of every session.
tests/test_ingestion.py compares the scene packed in assets/ with them.

tests/golden/piz/*.exr: the reference's PIZ textures.  The two 512^2 files are copied as they
are; of the two 4096^2 files (2.7 and 1.4 MB) the first PIZ_ROWS scanlines are kept: the same
header with dataWindow.yMax lowered, a shorter offset table, and those chunks byte for byte.
"""
import os
import shutil
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]

import nart_amd  # noqa: E402
import oracle  # noqa: E402
from exr_py import PIZ, parse_header  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
SCENES = ["glassSphere", "ring", "veach"]
SCENE_SIZE = (40, 24, 2)
PIZ_WHOLE = ["glassIceWater/iceCube_normal.exr", "glassIceWater/iceCube_roughness.exr"]
PIZ_CROPPED = ["glassIceWater/glass_roughness.exr", "cameraLens/lens_roughness.exr"]
PIZ_ROWS = 1024


def scene_golden(ref, name):
    cwd = os.getcwd()
    os.chdir(ref)  # the reference's paths are relative to its root ("input//meshes//...")
    try:
        rel = os.path.join("input", "scenes", name + ".json")
        orig = nart_amd.Scene(rel)
        sessions = nart_amd.load_sessions(rel)
    finally:
        os.chdir(cwd)
    c = orig.counts()
    out = {"counts": np.array([c[k] for k in sorted(c)], np.uint32),
           "sessions": np.stack([np.frombuffer(bytes(p), np.uint8) for p in sessions])}
    for k, p in enumerate(sessions):
        p.image_width, p.image_height, p.spp = SCENE_SIZE
        out["image_%d" % k] = oracle.Oracle(orig).render(p)
    np.savez_compressed(os.path.join(GOLDEN, "reference_scene_%s.npz" % name), **out)
    print(name, c, "%d session(s)" % len(sessions))


def crop_exr(src, dst, rows):
    buf = open(src, "rb").read()
    hdr, pos = parse_header(buf)
    assert hdr["compression"] == PIZ
    xmin, ymin, xmax, ymax = hdr["window"]
    lines = 32
    assert rows % lines == 0 and rows <= ymax - ymin + 1
    n_all, n = (ymax - ymin + lines) // lines, rows // lines
    offsets = struct.unpack_from("<%dQ" % n_all, buf, pos)
    chunks = []
    for off in offsets:
        y, size = struct.unpack_from("<ii", buf, off)
        if y - ymin < rows:
            chunks.append((y, buf[off:off + 8 + size]))
    chunks.sort()
    assert len(chunks) == n
    head = bytearray(buf[:pos])
    at = head.index(b"dataWindow\0box2i\0") + len(b"dataWindow\0box2i\0") + 4
    assert struct.unpack_from("<iiii", head, at) == (xmin, ymin, xmax, ymax)
    struct.pack_into("<iiii", head, at, xmin, ymin, xmax, ymin + rows - 1)
    table, body, at = [], b"", pos + 8 * n
    for _, c in chunks:
        table.append(at + len(body))
        body += c
    with open(dst, "wb") as f:
        f.write(bytes(head) + struct.pack("<%dQ" % n, *table) + body)
    print(os.path.basename(dst), "%d of %d rows, %d bytes" % (rows, ymax - ymin + 1, os.path.getsize(dst)))


def main(ref):
    for name in SCENES:
        scene_golden(ref, name)
    os.makedirs(os.path.join(GOLDEN, "piz"), exist_ok=True)
    tex = os.path.join(ref, "input", "textures")
    for rel in PIZ_WHOLE:
        shutil.copyfile(os.path.join(tex, rel), os.path.join(GOLDEN, "piz", os.path.basename(rel)))
    for rel in PIZ_CROPPED:
        crop_exr(os.path.join(tex, rel), os.path.join(GOLDEN, "piz", os.path.basename(rel)), PIZ_ROWS)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
