"""bench.py's plain run: the result line carries the headline fields and ms_per_step, nothing that
belongs to --full, and --dump-outputs writes the framebuffer of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_outputs(gpu, glass_scene, tmp_path):
    import nart_amd
    out = str(tmp_path / "outputs")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--size", "200x120x8",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", out],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    # value is the samples of the timed steps over their wall time
    assert line["value"] == pytest.approx(200 * 120 * 8 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    for key in ("roofline", "cpu_baseline", "parity", "counters_per_sample", "image_finite"):
        assert key not in line
    assert os.listdir(out) == ["image.npy"]
    img = np.load(os.path.join(out, "image.npy"))
    assert img.dtype == np.float32
    p = nart_amd.load_sessions(glass_scene.path)[0]
    p.image_width, p.image_height, p.spp = 200, 120, 8
    ref = nart_amd.HipRenderer(glass_scene).render(p)
    assert img.shape == ref.shape and np.array_equal(img.view(np.uint32), ref.view(np.uint32))
