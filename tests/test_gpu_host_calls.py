"""The host-buffer calls share one scaffold (vr_host.h HostCall): a pooled call context whose scratch
buffer every call lays out for itself.  Calls of different kinds and sizes, made one after another
from one thread, are all served by the same context; each must give, bit for bit, what the same call
gives on a freshly created scene, whose context has never held anything else.

The sizes cross every branch of the layout: n not a multiple of 16, n = 1, scratch growing, shrinking
and growing again, optional arrays absent, and vr_render_tile's one-sample-into-a-fresh-buffer path.
"""
import numpy as np
import pytest

from vanrijn_amd import scenes
from vanrijn_amd.render import (Film, Tile, camera_rays_device, integrate_rays, query_any, query_closest,
                                render_samples, render_tile, trace_rays)

pytestmark = pytest.mark.gpu

H = W = 16
FULL = Tile(0, 16, 0, 16)
SEED = 0x5CA1AB1E


def _scene():
    return scenes.main_scene(scenes.procedural_bunny(12))


def _raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _buffer(b):
    return [b.colour_buffer, b.colour_sum_buffer, b.colour_bias_buffer, b.weight_buffer, b.weight_bias_buffer]


@pytest.fixture(scope="module")
def rays():
    """4,099 rays: the camera rays of the 16 x 16 image at 16 spp (sample-major, so every prefix of 256
    covers the whole image), then three that start above everything and point up."""
    import torch
    n = 16 * 16 * 16
    o = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
    d = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
    ids = torch.zeros(n, dtype=torch.int64, device="cuda")
    camera_rays_device(_scene(), FULL, H, W, 16, SEED, 0, o.data_ptr(), d.data_ptr(), ids.data_ptr())
    torch.cuda.synchronize()
    up = np.array([[0.0, 50.0, 0.0], [3.0, 60.0, -2.0], [-4.0, 70.0, 1.0]])
    cam_o, cam_d = o.cpu().numpy().reshape(-1, 3), d.cpu().numpy().reshape(-1, 3)

    def take(n):
        k = n - 3 if n > 3 else n
        o_n = np.concatenate([cam_o[:k], up[:n - k]])
        d_n = np.concatenate([cam_d[:k], np.tile([0.0, 1.0, 0.0], (n - k, 1))])
        return np.ascontiguousarray(o_n), np.ascontiguousarray(d_n)
    return take


def _calls(rays):
    """(name, call): each call takes a scene and returns the arrays it produced."""
    def film(s):
        with Film(W, H) as f:
            f.render_tile(s, FULL, 2, SEED + 3)
            return _buffer(f.read()[0])

    def integrate(s):
        o, d = rays(33)
        return list(integrate_rays(s, o, d, SEED, wavelengths=np.linspace(400.0, 700.0, 33), info=True))

    first = ("render_tile 16x16 2spp", lambda s: _buffer(render_tile(s, FULL, H, W, 2, SEED)))
    return [
        first,
        ("query_any 257", lambda s: [query_any(s, *rays(257))]),
        ("integrate_rays 33", integrate),
        ("render_samples 5x3 3spp", lambda s: [render_samples(s, Tile(3, 8, 5, 8), H, W, 3, SEED + 1)]),
        ("trace_rays 1", lambda s: [trace_rays(s, *rays(1))]),
        ("query_closest 4099 records", lambda s: list(query_closest(s, *rays(4099), records=True))),
        ("render_tile 8x8 1spp fresh", lambda s: _buffer(render_tile(s, Tile(4, 12, 4, 12), H, W, 1, SEED + 2))),
        ("film 16x16", film),
        ("render_tile 16x16 2spp again", first[1]),
    ]


def test_calls_sharing_one_context_match_fresh_scenes(rays):
    shared = _scene()
    got = {}
    for name, call in _calls(rays):
        got[name] = call(shared)  # one thread: the scene's one pooled context serves every call
        want = call(_scene())
        assert len(got[name]) == len(want)
        for k, (a, b) in enumerate(zip(got[name], want)):
            assert np.array_equal(_raw(a), _raw(b)), (name, k)
    for a, b in zip(got["render_tile 16x16 2spp"], got["render_tile 16x16 2spp again"]):
        assert np.array_equal(_raw(a), _raw(b))
    # the comparison is not one of empty buffers: the any-hit set is mixed (as test_any_hit_set_is_mixed
    # shows for this scene), hits carry records, and the renders hold light
    any_hit = got["query_any 257"][0]
    assert any_hit[:254].sum() >= 16 and (~any_hit[:254]).sum() >= 16 and not any_hit[254:].any()
    hits, rec = got["query_closest 4099 records"]
    assert 400 < hits["valid"].sum() < 3700 and np.array_equal(hits["valid"], rec["valid"])
    assert got["trace_rays 1"][0]["valid"][0] == hits["valid"][0]
    assert (got["render_tile 16x16 2spp"][3] == 2.0).all() and got["render_tile 16x16 2spp"][1].any()
    assert (got["render_tile 8x8 1spp fresh"][3] == 1.0).all() and got["film 16x16"][0].any()
