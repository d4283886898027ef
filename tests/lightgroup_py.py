"""Light groups (include/nart_hip.h, "Light groups") restated for the tests: the mix in numpy float32,
the scene files whose lights are switched off by intensity 0 -- the yardstick the group images are
compared with: the unchanged oracle on an edited scene file -- and the frames the tests share."""
import json
import os

import numpy as np

f32 = np.float32
GROUPS_MAX = 8


def mix(images, gains):
    """out = mix(groups, gains[G][3]): per pixel and channel c of r, g, b
    acc = 0.f; for g ascending: acc = acc + gains[g][c] * I_g[c], float32, unfused, in this order;
    alpha and filter weight sum copied from image 0."""
    images = np.asarray(images, f32)
    gains = np.asarray(gains, f32)
    if gains.ndim == 1:
        gains = np.repeat(gains[:, None], 3, axis=1)
    assert images.ndim == 4 and images.shape[-1] == 5 and gains.shape == (images.shape[0], 3)
    out = np.empty(images.shape[1:], f32)
    with np.errstate(all="ignore"):
        acc = np.zeros(images.shape[1:3] + (3,), f32)
        for g in range(images.shape[0]):
            prod = (gains[g][None, None, :] * images[g][..., :3]).astype(f32)  # one rounding
            acc = (acc + prod).astype(f32)                                     # and another
    out[..., :3] = acc
    out[..., 3:] = images[0][..., 3:]
    return out


def scene_with(path, out_path, lit=None, extra_lights=(), session=None):
    """The scene file `path` written again as `out_path`: `extra_lights` appended, then every light whose
    index is not in `lit` (None: all stay lit) given intensity 0; `session` updates the first render
    session.  Returns out_path."""
    with open(path) as f:
        scene = json.load(f)
    scene["lights"] = list(scene["lights"]) + [dict(l) for l in extra_lights]
    if lit is not None:
        for i, l in enumerate(scene["lights"]):
            if i not in lit:
                l["intensity"] = 0.0
    if session:
        scene["renderSessions"][0].update(session)
    with open(out_path, "w") as f:
        json.dump(scene, f, indent=1)
    return out_path


# a disk light above the scene, facing down: appended to the scenes that have one light
DISK = {"type": "disk", "radius": 0.6, "Le": [1.0, 0.8, 0.6], "intensity": 25.0,
        "transform": [1, 0, 0, 0.5, 0, 1, 0, -0.5, 0, 0, 1, 3.5, 0, 0, 0, 1]}


def n_lights(path):
    with open(path) as f:
        return len(json.load(f)["lights"])


def sum_bound(spp, filter_width, bounces, G):
    """|sum_g I_g - B| <= (spp (2 ceil(fw) + 1)^2 + bounces + G + 2) 2^-23 sum_g I_g per pixel and channel:
    two orders of summing the same non-negative terms (each sample's at most bounces + 1 terms, then the
    splat's at most spp (2 ceil(fw) + 1)^2 samples per pixel, then the G images)."""
    return (spp * (2 * int(np.ceil(filter_width)) + 1) ** 2 + bounces + G + 2) * 2.0 ** -23


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def bits_equal(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def report(a, b):
    ne = bits(a) != bits(b)
    idx = np.argwhere(ne)
    with np.errstate(all="ignore"):
        worst = float(np.nanmax(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if ne.any() else 0.0
    return "%d of %d floats differ, max abs diff %g, first at %s" % (int(ne.sum()), ne.size, worst,
                                                                     idx[0].tolist() if len(idx) else None)


class Frames:
    """The scenes of the light-group tests and the oracle's zero-intensity frames of them, made once per
    test session and shared read-only.  base: {name: scene json path}; directory: where the edited scene
    files go."""

    def __init__(self, directory, base):
        self.dir = directory
        self.base = dict(base)
        self._scenes = {}
        self._frames = {}

    def path(self, name, lit=None):
        """The scene file of `name` with only the lights in `lit` on (None: the scene as it is)."""
        if lit is None:
            return self.base[name]
        out = os.path.join(self.dir, "%s_lit_%s.json" % (name, "_".join(map(str, sorted(lit)))))
        if not os.path.exists(out):
            scene_with(self.base[name], out, lit=set(lit))
        return out

    def scene(self, name, lit=None):
        import nart_amd
        k = (name, None if lit is None else tuple(sorted(lit)))
        if k not in self._scenes:
            self._scenes[k] = nart_amd.Scene(self.path(name, lit))
        return self._scenes[k]

    def params(self, name, w, h, spp, **kw):
        import nart_amd
        p = nart_amd.load_sessions(self.base[name])[0]
        p.image_width, p.image_height, p.spp = w, h, spp
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def oracle(self, name, p, lit=None):
        """The oracle's frame of `name` at p with only the lights in `lit` on."""
        import oracle
        k = (name, None if lit is None else tuple(sorted(lit)), p.image_width, p.image_height, p.spp, p.bucket_size,
             p.filter_width, p.bounces)
        if k not in self._frames:
            img = oracle.Oracle(self.scene(name, lit)).render(p)
            img.setflags(write=False)
            self._frames[k] = img
        return self._frames[k]


_shared = []


def shared_frames(tmp_path_factory):
    """The Frames of the test session over the suite's scenes: materials (ring + disk), veach (4 disks),
    ring (2 lights), environment with a textured and with a constant sky and nested glass (bounces 16),
    the last three with DISK appended."""
    if not _shared:
        from nart_amd import scenes
        d = str(tmp_path_factory.mktemp("light_groups"))
        sub = lambda n: os.path.join(d, n)  # noqa: E731
        base = {"materials": scenes.materials(sub("materials")), "veach": scenes.reference_scene("veach", sub("veach")),
                "ring": scenes.reference_scene("ring", sub("ring")),
                "env": scene_with(scenes.environment(sub("env")), sub("env_disk.json"), extra_lights=[DISK]),
                "envc": scene_with(scenes.environment(sub("envc"), textured_env=False), sub("envc_disk.json"),
                                   extra_lights=[DISK]),
                "nested": scene_with(scenes.nested_glass(sub("nested"), bounces=16), sub("nested_disk.json"),
                                     extra_lights=[DISK])}
        _shared.append(Frames(d, base))
    return _shared[0]


# The frames the definition was checked on (tests/test_light_groups_definition.py) and the GPU compares
# (tests/test_gpu_light_groups.py): name -> (width, height, spp)
DEFINITION_FRAMES = {"materials": (48, 32, 8), "veach": (48, 32, 8), "ring": (48, 32, 8), "env": (48, 32, 8),
                     "envc": (48, 32, 8), "nested": (48, 36, 4)}
