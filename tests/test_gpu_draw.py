"""The colours and the raster on the GPU (csrc/em2_draw.hip) against tests/native/em2_draw_restatement.cpp, which
tests/test_draw_cpu.py holds against an independent Python statement: the packed colours and the range equal, vertexTop and
edgeHits word for word, the composed image byte for byte.  S = 64 unless a case needs more; the view is [0, 64) x [0, 64), so a
unit is a pixel."""
import numpy as np
import pytest

import draw_binding as db
import test_draw_cpu as cpu
from expressionmatrix2_amd import capi

pytestmark = pytest.mark.gpu

S = 64
VIEW = (S, 32., 32., 32.)                   # size, centre, half size: a unit is a pixel, pixel i covers [i, i + 1)
U32 = np.uint32


@pytest.fixture(scope="module")
def restatement():
    return db.load()


def same_layers(restatement, x, y, v0, v1, view, radius, hide=False, what=""):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    v0, v1 = np.asarray(v0, dtype=U32), np.asarray(v1, dtype=U32)
    mine = capi.graph_draw(x, y, v0, v1, *view, radius, hide)
    theirs = restatement.graph_draw(x, y, v0, v1, *view, radius, hide)
    assert theirs is not None, what
    assert np.array_equal(mine[0], theirs[0]), "%s: vertexTop differs at %s" % (what, np.argwhere(mine[0] != theirs[0])[:5].tolist())
    assert np.array_equal(mine[1], theirs[1]), "%s: edgeHits differs at %s" % (what, np.argwhere(mine[1] != theirs[1])[:5].tolist())
    return mine


# ---- colours ----

@pytest.mark.parametrize("name", sorted(cpu.color_cases()))
def test_colours_equal_the_restatement(restatement, name):
    values, low, high = cpu.color_cases()[name]
    rgb, value_range = capi.spectral_colors(values, low, high)
    expected, expected_range = restatement.spectral_colors(values, low, high)
    assert np.array_equal(rgb, expected), name
    assert np.array_equal(value_range, expected_range), name              # (0. == -0.: the sign of a zero bound is not pinned)


def test_colours_over_more_than_one_block(restatement):
    """70 001 values: 274 blocks of partial bounds, the extremes in the last, partial one; a NaN and a "no value" among them."""
    rng = np.random.default_rng(5)
    values = rng.random(70001) * 3. - 1.
    values[70000], values[69990], values[17], values[40000] = -7.25, 11.5, np.nan, db.NO_VALUE
    for low, high in ((None, None), (0., 1.), (None, 2.)):
        rgb, value_range = capi.spectral_colors(values, low, high)
        expected, expected_range = restatement.spectral_colors(values, low, high)
        assert np.array_equal(rgb, expected) and np.array_equal(value_range, expected_range)
        assert value_range[0] == -7.25 and value_range[1] == 11.5 and rgb[17] == 0x00ff00 and rgb[40000] == db.COLOR_NONE
    assert capi.color_strings(rgb[[70000, 69990, 17, 40000]]) == ["#ff0000", "#00ff00", "#00ff00", ""]


def test_pinned_colours():
    strings = lambda values, *bounds: capi.color_strings(capi.spectral_colors(np.asarray(values, dtype=np.float64), *bounds)[0])
    assert strings([0., 0.5, 1.]) == ["#ff0000", "#ffff00", "#00ff00"]
    assert strings([-3., 9.], 0., 1.) == ["#ff0000", "#00ff00"]
    assert strings([1., np.nan, 3.]) == ["#ff0000", "#00ff00", "#00ff00"]
    assert strings([2.5, db.NO_VALUE, 2.5]) == ["black"] * 3 and strings([db.NO_VALUE] * 2) == ["black"] * 2
    assert strings([0., db.NO_VALUE, 1.]) == ["#ff0000", "", "#00ff00"] and strings([]) == []
    # value * 2 * 255 just below and on an integer
    on, below = 1. / 510., np.nextafter(1. / 510., 0.)
    assert int(2. * on * 255.) == 1 and int(2. * below * 255.) == 0
    assert strings([0., on, below, 0.25, 1.]) == ["#ff0000", "#ff0100", "#ff0000", "#ff7f00", "#00ff00"]


# ---- vertices ----

VERTEX_X = [10.5, 20., 0., 64., 63.999, -5., -0.001, 70., 40., 40., 1e30, -1e30, 32.25, 5., 61.]
VERTEX_Y = [10.5, 30., 0., 64., 63.999, 12., -0.001, 70., 41., 41., 5., 5., 1e30, 60., 3.]


@pytest.mark.parametrize("radius", (0., 1.5, 4., 4.01, 40., 256.))
def test_vertices(restatement, radius):
    """A vertex on a pixel centre, on a pixel boundary, on the view box's corner and edge, left / above and right / below the
    view, at +-1e30 (the clamp), two coincident ones (the later wins); radius 0, 1.5 px, the two sides of the lane / wave split,
    40 px across the border, and the cap."""
    none = np.zeros(0, dtype=U32)
    top, hits = same_layers(restatement, VERTEX_X, VERTEX_Y, none, none, VIEW, radius, what="radius %g" % radius)
    assert not hits.any()
    if radius == 0.:
        assert top[10, 10] == 1 and top[30, 20] == 2 and top[0, 0] == 3 and top[63, 63] == 5 and top[41, 40] == 10
        assert np.count_nonzero(top) == 7                       # 9 and 10 share a pixel; seven vertices lie outside
    if radius == 256.:
        assert (top > 0).all()


def test_sixty_five_vertices_on_one_pixel(restatement):
    none = np.zeros(0, dtype=U32)
    x = np.full(65, 17.3) + np.arange(65) * 0.01
    top, _ = same_layers(restatement, x, np.full(65, 9.5), none, none, VIEW, 0., what="65 on a pixel")
    assert top[9, 17] == 65 and np.count_nonzero(top) == 1
    top, _ = same_layers(restatement, x[::-1], np.full(65, 9.5), none, none, VIEW, 2., what="65 on a pixel, radius 2")
    assert top[9, 17] == 65


# ---- edges ----

def edge_case(*segments):
    x, y = [], []
    for x0, y0, x1, y1 in segments:
        x += [x0, x1]
        y += [y0, y1]
    ids = np.arange(len(x), dtype=U32)
    both = np.concatenate([ids[0::2], ids[1::2]]), np.concatenate([ids[1::2], ids[0::2]])        # every edge, and every edge reversed
    return np.array(x) + 0.5, np.array(y) + 0.5, both[0], both[1]


def test_edges_in_every_direction_and_reversed(restatement):
    """Horizontal, vertical, 45 degrees, steep, shallow, each reversed; a zero-length edge."""
    x, y, v0, v1 = edge_case((3, 5, 40, 5), (7, 2, 7, 50), (10, 10, 30, 30), (50, 2, 20, 32), (12, 3, 19, 60), (3, 40, 60, 47),
                             (60, 60, 33, 50), (45, 25, 45, 25), (2, 62, 3, 61))
    top, hits = same_layers(restatement, x, y, v0, v1, VIEW, 0., what="directions")
    assert hits[5, 3] == 2 and hits[5, 40] == 2 and hits[5, 41] == 0 and hits[25, 45] == 2 and hits[20, 20] == 2
    # an edge and its reverse are not the same pixels in general (the rounding of the minor axis): the sum is what is compared
    assert hits.sum() == 2 * (38 + 49 + 21 + 31 + 58 + 58 + 28 + 1 + 2)


def test_edges_that_leave_the_image(restatement):
    """Both ends outside with the line crossing the image and without; one end outside on every side; one end 10^6 pixels away
    in every direction; ends at the clamp."""
    far = 1e6
    x, y, v0, v1 = edge_case((-20, 10, 90, 50), (-20, -5, 90, -30), (-10, 80, 80, -10), (70, 70, 200, 90), (-30, 30, -2, 35),
                             (30, -40, 33, 120), (10, 10, -7, 3), (10, 10, 70, 12), (50, 50, 55, 99), (50, 50, 44, -9),
                             (32, 32, far, 40), (32, 32, -far, 17), (5, 60, 77, far), (5, 60, 31, -far), (far, far, 3, 4),
                             (-far, 10, far, 50), (1e30, 1e30, 10, 10), (-1e30, 20, 1e30, 20), (63, 0, 64, 0), (0, 63, -1, 64))
    top, hits = same_layers(restatement, x, y, v0, v1, VIEW, 0., what="clipping")
    assert hits.any() and (hits[20] >= 2).all()


def test_edges_around_the_cut_off(restatement):
    """Edges of exactly the cut-off, cut-off +- 1 and 10 x cut-off steps inside the image, shallow and steep, in both directions,
    whole inside and cut by the border; S = 1024 so that the longest fits."""
    cut = capi.graph_draw_long_edge_steps()
    assert 16 <= cut <= 100
    segments = []
    for at, steps in enumerate((cut - 1, cut, cut + 1, 10 * cut, 2 * cut + 1)):
        extent = steps - 1                                      # dM + 1 steps
        segments += [(5, 10 + 20 * at, 5 + extent, 17 + 20 * at), (300 + 20 * at, 5, 309 + 20 * at, 5 + extent)]
        # from outside: `steps` steps lie inside
        segments += [(-50, 200 + 20 * at, steps - 1, 211 + 20 * at), (500 + 20 * at, 1023 + 80, 503 + 20 * at, 1024 - steps)]
    x, y, v0, v1 = edge_case(*segments)
    view = (1024, 512., 512., 512.)
    top, hits = same_layers(restatement, x, y, v0, v1, view, 0., what="cut-off")
    assert hits.sum() == 2 * 4 * sum((cut - 1, cut, cut + 1, 10 * cut, 2 * cut + 1))


def test_a_hundred_edges_through_one_pixel(restatement):
    angles = np.arange(100) * (2. * np.pi / 100.)
    x = np.concatenate([[32.5], 32.5 + 25. * np.cos(angles)])
    y = np.concatenate([[32.5], 32.5 + 25. * np.sin(angles)])
    v0, v1 = np.zeros(100, dtype=U32), np.arange(1, 101, dtype=U32)
    top, hits = same_layers(restatement, x, y, v0, v1, VIEW, 0., what="star")
    assert hits[32, 32] == 100
    # 100 long edges over one another: every pixel of a row 100 times, by the wave path
    size = 2 * capi.graph_draw_long_edge_steps()
    x, y = np.array([-3., size + 9.]), np.array([7.5, 7.5])
    top, hits = same_layers(restatement, x, y, np.zeros(100, dtype=U32), np.ones(100, dtype=U32), (size, size / 2., size / 2., size / 2.),
                            0., what="stack")
    assert (hits[7] == 100).all() and hits.sum() == 100 * size


def test_hidden_and_absent_edges(restatement):
    x, y, v0, v1 = edge_case((3, 5, 40, 5), (-20, 10, 90, 50))
    top, hits = same_layers(restatement, x, y, v0, v1, VIEW, 1.5, hide=True, what="hideEdges")
    assert not hits.any() and top.any()
    none = np.zeros(0, dtype=U32)
    top, hits = same_layers(restatement, x, y, none, none, VIEW, 1.5, what="edgeCount 0")
    assert not hits.any() and top.any()
    top, hits = same_layers(restatement, np.zeros(0), np.zeros(0), none, none, VIEW, 1.5, what="nothing at all")
    assert not hits.any() and not top.any()


def test_random_graph_at_an_odd_size(restatement):
    rng = np.random.default_rng(9)
    n, m = 700, 3000
    x, y = rng.random(n) * 120. - 10., rng.random(n) * 120. - 10.
    v0, v1 = rng.integers(0, n, m).astype(U32), rng.integers(0, n, m).astype(U32)
    for radius in (0.8, 7.3):
        same_layers(restatement, x, y, v0, v1, (97, 51.3, 48.9, 55.5), radius, what="random, radius %g" % radius)


def test_one_pixel_image(restatement):
    x, y = np.array([0.5, 0.2, 7., -3.]), np.array([0.5, 0.9, 0.5, 0.5])
    top, hits = same_layers(restatement, x, y, [0, 0, 2, 2], [1, 2, 3, 0], (1, 0.5, 0.5, 0.5), 0.1, what="S = 1")
    assert top.shape == (1, 1) and top[0, 0] == 2 and hits[0, 0] == 4


def test_errors_leave_the_outputs_untouched():
    x, y = np.array([1., 2., 3.]), np.array([1., 2., 3.])
    v0, v1 = np.array([0, 1], dtype=U32), np.array([1, 2], dtype=U32)
    top, hits = np.full((S, S), 0x5a5a5a5a, dtype=U32), np.full((S, S), 0x5a5a5a5a, dtype=U32)
    bad_x = x.copy()
    bad_x[2] = np.nan
    bad_y = y.copy()
    bad_y[0] = -np.inf
    for what, arguments in (("a NaN position", (bad_x, y, v0, v1, *VIEW, 1.5)), ("an infinite position", (x, bad_y, v0, v1, *VIEW, 1.5)),
                            ("halfSize 0", (x, y, v0, v1, S, 32., 32., 0., 1.5)), ("halfSize -1", (x, y, v0, v1, S, 32., 32., -1., 1.5)),
                            ("halfSize inf", (x, y, v0, v1, S, 32., 32., np.inf, 1.5)), ("halfSize NaN", (x, y, v0, v1, S, 32., 32., np.nan, 1.5)),
                            ("a radius above the cap", (x, y, v0, v1, *VIEW, 256.01)), ("a negative radius", (x, y, v0, v1, *VIEW, -1.)),
                            ("an edge end out of range", (x, y, v0, np.array([1, 3], dtype=U32), *VIEW, 1.5))):
        with pytest.raises(RuntimeError, match="em2_graph_draw"):
            capi.graph_draw(*arguments, vertex_top=top, edge_hits=hits)
        assert (top == 0x5a5a5a5a).all() and (hits == 0x5a5a5a5a).all(), what
    for size in (0, 8193):
        with pytest.raises(RuntimeError, match="sizePixels"):
            capi.graph_draw(x, y, v0, v1, size, 32., 32., 32., 1.5)
    capi.graph_draw(x, y, v0, v1, *VIEW, 256., vertex_top=top, edge_hits=hits)           # the cap itself is allowed
    assert (top == 3).all()


# ---- compose ----

def test_compose_every_priority_and_shade(restatement):
    rng = np.random.default_rng(4)
    top = rng.integers(0, 6, (S, S)).astype(U32) * (rng.random((S, S)) < 0.5)
    hits = rng.integers(0, 400, (S, S)).astype(U32) * (rng.random((S, S)) < 0.5)
    top[0, :4] = [0, 0, 1, 2]
    hits[0, :4] = [0, 3, 0, 3]
    rgb = np.array([0x123456, db.COLOR_NONE, db.COLOR_BLACK, 0xffffff, 0x00ff00], dtype=U32)
    for shade in (1, 100, 255):
        image = capi.graph_compose(top, hits, rgb, shade)
        assert np.array_equal(image, restatement.graph_compose(top, hits, rgb, shade)), shade
        assert image[0, 0].tolist() == [255] * 4 and image[0, 1].tolist() == [255 - min(255, 3 * shade)] * 3 + [255]
        assert image[0, 2].tolist() == [0x12, 0x34, 0x56, 255] and image[0, 3].tolist() == [0, 0, 0, 255]
    assert np.array_equal(capi.graph_compose(top, hits, None, 255), restatement.graph_compose(top, hits, np.zeros(5, dtype=U32), 255))
    with pytest.raises(RuntimeError, match="edgeShade"):
        capi.graph_compose(top, hits, rgb, 0)
    with pytest.raises(RuntimeError, match="edgeShade"):
        capi.graph_compose(top, hits, rgb, 256)
    with pytest.raises(RuntimeError, match="above vertexCount"):
        capi.graph_compose(top, hits, rgb[:4], 255)


def test_device_entries_equal_the_host_forms(restatement):
    """em2_dev_graph_draw, em2_dev_spectral_colors and em2_dev_graph_compose on device memory, one after the other."""
    import torch
    lib = capi.load()
    rng = np.random.default_rng(12)
    n, m, size = 300, 900, 80
    x, y = rng.random(n) * 100. - 10., rng.random(n) * 100. - 10.
    v0, v1 = rng.integers(0, n, m).astype(U32), rng.integers(0, n, m).astype(U32)
    values = rng.random(n)
    values[7] = db.NO_VALUE
    device = lambda a, kind: torch.from_numpy(np.ascontiguousarray(a).view(kind).copy()).cuda()
    d_x, d_y, d_values = device(x, np.float64), device(y, np.float64), device(values, np.float64)
    d_v0, d_v1 = device(v0, np.int32), device(v1, np.int32)
    d_top = torch.full((size, size), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_hits = torch.full((size, size), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_range = torch.zeros(4, dtype=torch.float64, device="cuda")
    d_rgba = torch.zeros((size, size), dtype=torch.int32, device="cuda")
    draw_bytes, color_bytes = lib.em2_dev_graph_draw_workspace(n, m), lib.em2_dev_spectral_colors_workspace()
    d_workspace = torch.zeros(max(draw_bytes, color_bytes), dtype=torch.uint8, device="cuda")
    view = (size, 40., 41., 45., 2.6)

    def draw(d_edge_end, workspace_bytes=draw_bytes):
        return lib.em2_dev_graph_draw(n, d_x.data_ptr(), d_y.data_ptr(), m, d_v0.data_ptr(), d_edge_end.data_ptr(), 0, *view, d_top.data_ptr(),
                                      d_hits.data_ptr(), d_workspace.data_ptr(), workspace_bytes, None)

    bad = v1.copy()
    bad[m - 1] = n                                                # found by the kernel: nothing may be written
    assert draw(device(bad, np.int32)) == capi.EM2_ERROR_INVALID_ARGUMENT and "not below vertexCount" in capi.last_error()
    assert draw(d_v1, draw_bytes - 1) == capi.EM2_ERROR_INVALID_ARGUMENT
    assert (d_top == 0x5a5a5a5a).all().item() and (d_hits == 0x5a5a5a5a).all().item()
    capi.check(draw(d_v1))
    top, hits = d_top.cpu().numpy().view(U32), d_hits.cpu().numpy().view(U32)
    expected = restatement.graph_draw(x, y, v0, v1, *view)
    assert np.array_equal(top, expected[0]) and np.array_equal(hits, expected[1])
    capi.check(lib.em2_dev_spectral_colors(d_values.data_ptr(), n, 0.25, 0., 1, 0, d_rgb.data_ptr(), d_range.data_ptr(),
                                           d_workspace.data_ptr(), color_bytes, None))
    capi.check(lib.em2_dev_graph_compose(size, d_top.data_ptr(), d_hits.data_ptr(), d_rgb.data_ptr(), 100, d_rgba.data_ptr(), None))
    torch.cuda.synchronize()
    rgb, value_range = restatement.spectral_colors(values, 0.25, None)
    assert np.array_equal(d_rgb.cpu().numpy().view(U32), rgb) and np.array_equal(d_range.cpu().numpy(), value_range)
    image = d_rgba.cpu().numpy().view(np.uint8).reshape(size, size, 4)
    assert np.array_equal(image, restatement.graph_compose(top, hits, rgb, 100))
