"""The colour census and the raster with pies on the GPU (csrc/em2_pie.hip) against
tests/native/em2_signature_draw_restatement.cpp, which tests/test_signature_draw_cpu.py holds against an independent Python
statement: the four arrays of the census bit for bit, vertexTop, sliceTop and edgeHits word for word, the composed image byte
for byte against draw_binding.python_compose."""
import ctypes

import numpy as np
import pytest

import draw_binding as db
import signature_draw_binding as sb
import test_signature_draw_cpu as cpu
from expressionmatrix2_amd import capi

pytestmark = pytest.mark.gpu

U32 = np.uint32
KEYS = ("sliceOffsets", "sliceColor", "sliceCells", "sliceFraction")


@pytest.fixture(scope="module")
def restatement():
    return sb.load()


# ---- the census ----

def test_the_threshold_the_cases_sit_around():
    assert capi.pie_census_wave_cells() == cpu.WAVE_CELLS
    assert capi.graph_draw_pies_wave_radius() == 32.


@pytest.mark.parametrize("name", sorted(cpu.census_cases()))
def test_census_equals_the_restatement(restatement, name):
    case = cpu.census_cases()[name]
    mine, theirs = capi.pie_census(*case), restatement.census(*case)
    for key in KEYS:
        assert mine[key].dtype == theirs[key].dtype and mine[key].tobytes() == theirs[key].tobytes(), (name, key)
    assert mine["waveVertexCount"] == int((np.diff(case[0].astype(np.int64)) > cpu.WAVE_CELLS).sum())
    assert mine["values"] == [] and mine["valueCells"] == []


def test_census_refuses_an_id_out_of_range():
    offsets, cells, ids, colors = cpu.census_case([[0, 1], [2] * 40, [1]])
    lib = capi.load()

    def refused(offsets, cells, ids, colors):
        handle = ctypes.c_void_p(None)
        rc = lib.em2_pie_census_create(len(offsets) - 1, capi._ptr(offsets), capi._ptr(cells), len(cells), capi._ptr(ids), len(ids),
                                       capi._ptr(colors), len(colors), ctypes.byref(handle))
        return rc == capi.EM2_ERROR_INVALID_ARGUMENT and handle.value is None and "em2_pie_census" in capi.last_error()

    bad = ids.copy()
    bad[cells[1]] = 3                                            # a lane's vertex
    assert refused(offsets, cells, bad, colors)
    bad = ids.copy()
    bad[cells[30]] = 0xffffffff                                  # a wave's vertex
    assert refused(offsets, cells, bad, colors)
    far = cells.copy()
    far[41] = len(ids)
    assert refused(offsets, far, ids, colors)
    assert refused(offsets, cells, ids, np.array([0, 13, 2], dtype=np.uint8))
    assert refused(np.array([0, 2, 1, 43], dtype=np.uint64), cells, ids, colors)
    assert refused(np.array([0, 2, 42, 44], dtype=np.uint64), cells, ids, colors)
    assert capi.pie_census(offsets, cells, ids, colors)["sliceCells"].tolist() == [1, 1, 40, 1]


def test_census_on_device_memory(restatement):
    import torch
    lib = capi.load()
    case = cpu.census_cases()["random"]
    offsets, cells, ids, colors = case
    device = lambda a, kind: torch.from_numpy(np.ascontiguousarray(a).view(kind).copy()).cuda()
    d_offsets, d_cells, d_ids, d_colors = device(offsets, np.int64), device(cells, np.int32), device(ids, np.int32), device(colors, np.uint8)
    handle = ctypes.c_void_p(None)
    capi.check(lib.em2_dev_pie_census(len(offsets) - 1, d_offsets.data_ptr(), d_cells.data_ptr(), len(cells), d_ids.data_ptr(), len(ids),
                                      d_colors.data_ptr(), len(colors), ctypes.byref(handle)))
    mine, theirs = capi.pie_census_take(handle), restatement.census(*case)
    for key in KEYS:
        assert mine[key].tobytes() == theirs[key].tobytes(), key


# ---- the raster ----

def same_layers(restatement, case, what):
    mine = capi.graph_draw_pies(*case)
    theirs = restatement.graph_draw_pies(*case)
    assert theirs is not None, what
    for layer, a, b in zip(("vertexTop", "sliceTop", "edgeHits"), mine, theirs):
        assert np.array_equal(a, b), "%s: %s differs at %s" % (what, layer, np.argwhere(a != b)[:5].tolist())
    return mine


@pytest.mark.parametrize("name", sorted(cpu.raster_cases()))
def test_pies_equal_the_restatement(restatement, name):
    case = cpu.raster_cases()[name]
    top, slices, hits = same_layers(restatement, case, name)
    assert ((slices > 0) == (top > 0)).all()
    offsets = np.asarray(case[9]).astype(np.int64)
    covered = top > 0
    owner = np.searchsorted(offsets, slices[covered].astype(np.int64) - 1, side="right") - 1
    assert np.array_equal(owner, top[covered].astype(np.int64) - 1)               # a pixel's slice is one of its top vertex
    # a colour per slice, then the unchanged composition
    rgb = np.random.default_rng(1).integers(0, 1 << 24, int(offsets[-1])).astype(U32)
    for shade in (255, 40):
        assert np.array_equal(capi.graph_compose(slices, hits, rgb, shade), db.python_compose(slices, hits, rgb, shade)), name
    if name == "the whole image on top":
        assert (top == 8).all() and set(np.unique(slices).tolist()) == {int(offsets[7]) + 1, int(offsets[7]) + 2, int(offsets[7]) + 3}
    if name == "coincident boundaries":
        assert set(np.unique(slices[top == 1]).tolist()) == {2}              # slice 0 is empty: everything but ... is the last
        assert set(np.unique(slices[top == 2]).tolist()) == {3}              # slice 0 is the whole disc
    if name == "own pixel":
        assert slices[7, 10] == 1 and slices[9, 20] == 3 and np.count_nonzero(top) == 2
    if name == "one pixel":
        assert top.shape == (1, 1) and top[0, 0] == 2 and hits[0, 0] == 1


def test_pies_with_hidden_edges_and_without_vertices(restatement):
    case = list(cpu.raster_cases()["eight pies"])
    top, slices, hits = same_layers(restatement, tuple(case) + (True,), "hideEdges")
    assert not hits.any() and slices.any()
    none, nothing = np.zeros(0, dtype=U32), np.zeros(0)
    empty = (nothing, nothing, nothing, none, none, 64, 32., 32., 32., np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.int32),
             np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8))
    top, slices, hits = same_layers(restatement, empty, "no vertex")
    assert not top.any() and not slices.any() and not hits.any()


def test_pie_errors_leave_the_outputs_untouched():
    offsets, bx, by, arc = cpu.pie_slices([[0.5, 0.5], [1.], [0.2, 0.8]])
    x, y = np.array([5., 9., 30.]), np.array([5., 9., 31.])
    v0, v1 = np.array([0, 1], dtype=U32), np.array([1, 2], dtype=U32)
    layers = [np.full((64, 64), 0x5a5a5a5a, dtype=U32) for _ in range(3)]
    view = (64, 32., 32., 32.)

    def draw(x=x, radius=(1., 2., 3.), v1=v1, offsets=offsets, view=view):
        return capi.graph_draw_pies(x, y, radius, v0, v1, *view, offsets, bx, by, arc, vertex_top=layers[0], slice_top=layers[1],
                                    edge_hits=layers[2])

    bad_x = x.copy()
    bad_x[1] = np.nan
    for what, arguments, text in (("a NaN radius", dict(radius=(1., np.nan, 3.)), "radius"), ("an infinite radius", dict(radius=(np.inf, 2., 3.)), "radius"),
                                  ("a negative radius", dict(radius=(1., 2., -0.5)), "radius"), ("8193 pixels", dict(radius=(1., 8193., 3.)), "radius"),
                                  ("offsets that descend", dict(offsets=np.array([0, 3, 2, 5], dtype=np.uint64)), "sliceOffsets"),
                                  ("a vertex without a slice", dict(offsets=np.array([0, 2, 2, 5], dtype=np.uint64)), "sliceOffsets"),
                                  ("offsets past the slices", dict(offsets=np.array([0, 2, 3, 6], dtype=np.uint64)), "sliceOffsets"),
                                  ("a NaN position", dict(x=bad_x), "not finite"),
                                  ("an edge end out of range", dict(v1=np.array([1, 3], dtype=U32)), "not below vertexCount"),
                                  ("halfSize 0", dict(view=(64, 32., 32., 0.)), "viewBoxHalfSize")):
        with pytest.raises(RuntimeError, match="em2_graph_draw_pies.*" + text):
            draw(**arguments)
        assert all((layer == 0x5a5a5a5a).all() for layer in layers), what
    draw(radius=(1., 8192., 3.))                                 # the cap itself is allowed
    assert (layers[0] >= 2).all() and layers[2][5, 5] == 1


def test_pies_on_device_memory(restatement):
    import torch
    lib = capi.load()
    case = cpu.raster_cases()["random, S = 96"]
    x, y, radius, v0, v1, size, xc, yc, half, offsets, bx, by, arc = case
    device = lambda a, kind, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).view(kind).copy()).cuda()
    d = [device(x, np.float64, np.float64), device(y, np.float64, np.float64), device(radius, np.float64, np.float64),
         device(v0, np.int32, U32), device(v1, np.int32, U32), device(offsets, np.int64, np.uint64), device(bx, np.int32, np.int32),
         device(by, np.int32, np.int32), device(arc, np.uint8, np.uint8)]
    layers = [torch.full((size, size), 0x5a5a5a5a, dtype=torch.int32, device="cuda") for _ in range(3)]
    workspace_bytes = lib.em2_dev_graph_draw_pies_workspace(len(x), len(v0))
    workspace = torch.zeros(workspace_bytes, dtype=torch.uint8, device="cuda")

    def draw(bytes_given):
        return lib.em2_dev_graph_draw_pies(len(x), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(v0), d[3].data_ptr(), d[4].data_ptr(),
                                           0, size, xc, yc, half, d[5].data_ptr(), len(bx), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(),
                                           layers[0].data_ptr(), layers[1].data_ptr(), layers[2].data_ptr(), workspace.data_ptr(),
                                           bytes_given, None)

    assert draw(workspace_bytes - 1) == capi.EM2_ERROR_INVALID_ARGUMENT
    assert all((layer == 0x5a5a5a5a).all().item() for layer in layers)
    capi.check(draw(workspace_bytes))
    expected = restatement.graph_draw_pies(*case)
    for mine, theirs in zip(layers, expected):
        assert np.array_equal(mine.cpu().numpy().view(U32), theirs)
    d_rgb = torch.arange(len(bx), dtype=torch.int32, device="cuda") * 65793
    d_rgba = torch.zeros((size, size), dtype=torch.int32, device="cuda")
    capi.check(lib.em2_dev_graph_compose(size, layers[1].data_ptr(), layers[2].data_ptr(), d_rgb.data_ptr(), 255, d_rgba.data_ptr(), None))
    torch.cuda.synchronize()
    image = d_rgba.cpu().numpy().view(np.uint8).reshape(size, size, 4)
    assert np.array_equal(image, db.python_compose(expected[1], expected[2], d_rgb.cpu().numpy().view(U32), 255))
