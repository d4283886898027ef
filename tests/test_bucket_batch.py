"""How render_buckets cuts a bucket list into launches (csrc/host/bucket_batch.h gather_batch) and the slot
list of the per-sample entry points (append_rect), checked on the CPU against a numpy restatement.

A batch takes buckets in list order while their traced pixels fit the slot budget, the first always; a bucket
traces the pixels of its B x B square that lie inside the total image (the image grown by the filter bounds,
render.cpp:163-168), row by row, each packed as x | y << 16; `samples` counts only pixels inside the image."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("bucket_batch") / "bucket_batch_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "bucket_batch_check.cpp")])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return answers
    return ask


class Geometry:
    """nart_session_geometry of an image: the buckets tile the image, the total image adds the filter bounds."""

    def __init__(self, width, height, B, fb):
        self.W, self.H, self.B = width, height, B
        self.total_w, self.total_h = width + 2 * fb, height + 2 * fb
        self.nbx, self.nby = -(-width // B), -(-height // B)

    def pixels(self, bucket):
        """(xy, pixels inside the image) of a bucket."""
        bx, by = bucket % self.nbx, bucket // self.nbx
        xs = np.arange(self.B * bx, min(self.B * (bx + 1), self.total_w))
        ys = np.arange(self.B * by, min(self.B * (by + 1), self.total_h))
        x, y = np.meshgrid(xs, ys)  # row by row
        return (x | (y << 16)).ravel(), int(((x < self.W) & (y < self.H)).sum())

    def line(self, limit, ids):
        return "%d %d %d %d %d %d %d " % (self.B, self.nbx, self.total_w, self.total_h, self.W, self.H, limit) + \
            " ".join(map(str, ids))


def restate(g, ids, limit):
    """[(b1, counted so far, base, xy)] of the batches."""
    batches, b0, counted = [], 0, 0
    while b0 < len(ids):
        b1, base, xy = b0, [], []
        while b1 < len(ids):
            px, inside = g.pixels(ids[b1])
            if b1 > b0 and sum(map(len, xy)) + len(px) > limit:
                break
            base.append(sum(map(len, xy)))
            xy.append(px)
            counted += inside
            b1 += 1
        batches.append((b1, counted, base, np.concatenate(xy).tolist()))
        b0 = b1
    return batches


def _parse(line):
    out = []
    for batch in line.split(" ; "):
        b1, counted, base, xy = batch.split(" ")
        out.append((int(b1), int(counted), [int(v) for v in base.split(",")], [int(v) for v in xy.split(",")]))
    return out


# 40 x 30 at bucket 16, filter bounds 2: 3 x 2 buckets over a 44 x 34 total image; the right column is 12 wide (8
# inside the image), the bottom row has 14 of its 16 rows inside.  40 x 26: the bottom row is cut at the total
# height (14 rows, 10 inside) as well.
GEOMETRIES = [Geometry(40, 30, 16, 2), Geometry(40, 26, 16, 2)]
ORDERS = [[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [2, 2, 5, 0, 2, 5, 5, 1], [5], [0, 1, 0, 1]]
LIMITS = [1, 256, 511, 512, 12 * 16 + 256, 10 ** 6]  # 1; one bucket; a pixel short of two; two; a ragged one and a whole one


def test_gather_batch_matches_the_restatement(checker):
    cases = [(g, ids, limit) for g in GEOMETRIES for ids in ORDERS for limit in LIMITS]
    sizes = set()
    for (g, ids, limit), line in zip(cases, checker([g.line(limit, ids) for g, ids, limit in cases])):
        got, want = _parse(line), restate(g, ids, limit)
        assert got == want, (g.W, g.H, ids, limit)
        # every id in exactly one batch, in list order; a batch over the limit holds one bucket
        ends = [b[0] for b in got]
        assert ends == sorted(set(ends)) and ends[-1] == len(ids)
        b0 = 0
        for b1, counted, base, xy in got:
            lens = [len(g.pixels(i)[0]) for i in ids[b0:b1]]
            assert base == [sum(lens[:k]) for k in range(len(lens))] and len(xy) == sum(lens)  # the running offset
            assert len(xy) <= limit or b1 == b0 + 1
            if b1 < len(ids):  # the next bucket did not fit
                assert len(xy) + len(g.pixels(ids[b1])[0]) > limit
            assert counted == sum(g.pixels(i)[1] for i in ids[:b1])
            sizes.add(b1 - b0)
            b0 = b1
        if limit == 1:
            assert ends == list(range(1, len(ids) + 1))  # the first bucket is taken although it is over the limit
    assert {1, 2, 6} <= sizes


def test_ragged_buckets_and_counted(checker):
    g = GEOMETRIES[0]
    (b1, counted, base, xy), = _parse(checker([g.line(10 ** 6, range(6))])[0])
    assert b1 == 6 and counted == 40 * 30  # every image pixel once; the total image's margin is not counted
    assert len(xy) == 44 * 32 and base == [0, 256, 512, 704, 960, 1216]
    g = GEOMETRIES[1]
    (b1, counted, base, xy), = _parse(checker([g.line(10 ** 6, range(6))])[0])
    assert counted == 40 * 26 and len(xy) == 44 * 30


def test_append_rect(checker):
    got = [int(v) for v in checker(["rect 3 65530 4 3"])[0].split(",")]
    assert got == [x | (y << 16) for y in range(65530, 65533) for x in range(3, 7)]
