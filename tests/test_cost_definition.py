"""The definition of the cost record (include/nart_hip.h, "Cost image") rests on the unchanged oracle's
path counts (Oracle.render(p, counts=...)).  This checks, with the oracle alone and on every frame the GPU
test compares (cost_py.FRAMES), what that comparison needs: the grid formula gives the oracle's traced
samples; a zero bounce limit traces nothing; at a limit of one every sample traces its camera ray and
nothing more; at the session's limit the counts obey the record's invariants summed over the frame, and
some path continues, so that a kernel which counted camera rays alone could not pass."""
import pytest

import cost_py
import nart_amd


@pytest.fixture(scope="module")
def frames(built, tmp_path_factory):
    return cost_py.dc.lg.shared_frames(tmp_path_factory)


@pytest.mark.parametrize("key,spp", cost_py.FRAMES)
def test_oracle_counts(frames, key, spp):
    _name, p = cost_py.frame_params(frames, key, spp)
    gh, gw = cost_py.grid_shape(p, nart_amd.session_geometry(p))
    traced = gw * gh * spp
    zero = cost_py.oracle_counts(frames, key, spp, bounces=0)
    print(key, spp, "bounces 0:", zero)
    assert zero["extension_queries"] == zero["shaded_hits"] == zero["visibility_queries"] == 0
    one = cost_py.oracle_counts(frames, key, spp, bounces=1)
    print(key, spp, "bounces 1:", one)
    assert one["extension_queries"] == one["traced_samples"] == traced
    c = cost_py.oracle_counts(frames, key, spp)
    print(key, spp, "bounces %d:" % p.bounces, c)
    assert c["traced_samples"] == traced
    assert c["shaded_hits"] <= c["extension_queries"] <= p.bounces * traced
    assert c["visibility_queries"] <= 2 * c["shaded_hits"]
    assert c["extension_queries"] > traced  # some path continues


def test_grid_of_the_ragged_frame(frames):
    """materials 50x37 (bucket 16, filter width 1.5) traces 54x41 pixels: the filter's border too."""
    _name, p = cost_py.frame_params(frames, "materials_direct")
    g = nart_amd.session_geometry(p)
    assert cost_py.grid_shape(p, g) == (41, 54) == (g.total_height, g.total_width)
    _name, p = cost_py.frame_params(frames, "veach")
    assert cost_py.grid_shape(p, nart_amd.session_geometry(p)) == (32, 48)
