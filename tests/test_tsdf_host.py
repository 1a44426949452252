"""sfgs.tsdf without a GPU: the restatement tests/tsdf_np.py (what tests/test_gpu_tsdf.py holds the kernels to) gives a closed,
outward-wound, byte-weldable mesh of a sphere and an open one where the volume was not observed; the host build of the product's
csrc/tsdf_math.h (tests/host_check/tsdf_check.cpp) equals the restatement byte for byte on the shared scenes, winding table
included; the header, the library and the binding agree on the new symbols and structs with the ABI version unchanged; the
library and the wrapper refuse bad arguments before any GPU work; save_ply round-trips through a reader written here."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import tsdf_hostcheck as thc
import tsdf_np as tnp
from sfgs import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sfgs_tsdf_table_check", "sfgs_tsdf_integrate", "sfgs_tsdf_scratch_bytes", "sfgs_tsdf_extract")
E_ARG = -1


# ---- properties of the restatement -----------------------------------------------------------------------------------------------
def test_sphere_gives_a_closed_outward_mesh():
    tsdf, weight, _, origin, voxel = tnp.sphere_volume()
    verts, colors = tnp.extract(tsdf, weight, origin, voxel)
    assert colors is None and verts.dtype == np.float32 and verts.shape == (2012, 3, 3)
    r = tnp.mesh_report(verts)
    assert len(r.V) == 1008 and r.degenerate == 0
    assert (r.undirected == 2).all()                                          # closed: every edge between exactly two triangles
    assert (r.directed == 1).all()                                            # consistently wound: once in each direction
    assert r.euler == 2
    ratio = r.volume / (4.0 / 3.0 * np.pi * tnp.SPHERE.radius ** 3)
    print(f"signed volume {r.volume:.4f}, ratio to the sphere's {ratio:.5f}")
    # measured ON THE RESTATEMENT: +324.0275, ratio 0.97294 (linear cuts of a convex body lie inside it: below 1). The margin is
    # a radius error of 0.05 voxels: |dV / V| = 3 |dr| / r = 3 * 0.05 / 4.3 = 0.035.
    assert r.volume > 0 and abs(ratio - 0.973) < 0.035
    # every vertex lies within the linear cut's error of the sphere: at most len^2 / (8 r) = 3 / (8 * 4.3) = 0.087 on a body diagonal
    dist = np.linalg.norm(r.V.astype(np.float64) - np.array(tnp.SPHERE.centre), axis=1)
    assert np.abs(dist - tnp.SPHERE.radius).max() < 0.1


def test_unobserved_voxels_open_the_mesh_and_no_triangle_touches_an_unused_cell():
    tsdf, weight, _, origin, voxel = tnp.sphere_volume()
    weight = weight.copy()
    weight[5:8, 9:12, 6:9] = 0.0                                              # a block that straddles the surface
    verts, _ = tnp.extract(tsdf, weight, origin, voxel)
    full, _ = tnp.extract(tsdf, np.ones_like(weight), origin, voxel)
    assert 0 < len(verts) < len(full)
    r = tnp.mesh_report(verts)
    assert r.degenerate == 0 and set(r.undirected.tolist()) == {1, 2} and (r.directed == 1).all()
    # a cell is unused when one of its corners lies in the block: cells x 5..8, y 8..11, z 4..7 (voxel index = position here).
    # A triangle lies inside its cell, so its centroid names the cell.
    cell = np.floor(verts.astype(np.float64).mean(axis=1)).astype(int)
    bad = (cell[:, 0] >= 5) & (cell[:, 0] <= 8) & (cell[:, 1] >= 8) & (cell[:, 1] <= 11) & (cell[:, 2] >= 4) & (cell[:, 2] <= 7)
    assert not bad.any()
    cell_full = np.floor(full.astype(np.float64).mean(axis=1)).astype(int)
    gone = (cell_full[:, 0] >= 5) & (cell_full[:, 0] <= 8) & (cell_full[:, 1] >= 8) & (cell_full[:, 1] <= 11) & \
        (cell_full[:, 2] >= 4) & (cell_full[:, 2] <= 7)
    assert gone.sum() == len(full) - len(verts) > 0                           # exactly the block's triangles are missing
    assert full[~gone].tobytes() == verts.tobytes()                           # and the rest keeps its bytes and its order


def test_winding_bits_of_the_header_equal_the_geometric_derivation():
    lib = thc.lib()
    want = tnp.winding_table()
    assert want.shape == (6, 16) and 0 < want[:, 1:15].sum() < 6 * 14
    for t in range(6):
        assert [lib.tc_tet_corner(t, l) for l in range(4)] == list(tnp.TETS[t])
        for m in range(1, 15):
            assert lib.tc_winding_swap(t, m) == int(want[t, m]), (t, m)
    assert [lib.tc_tet_triangles(m) for m in range(16)] == [len(tnp.triangles_of(m)) for m in range(16)]
    # face diagonals match between neighbouring cells and all six tetrahedra share the body diagonal
    assert all(tet[0] == 0 and tet[3] == 7 for tet in tnp.TETS) and len(set(tnp.TETS)) == 6


def test_a_zero_value_is_outside_and_an_empty_volume_gives_nothing():
    tsdf = np.ones((3, 3, 3), np.float32)
    verts, _ = tnp.extract(tsdf, np.ones_like(tsdf), (0, 0, 0), 1.0)
    assert verts.shape == (0, 3, 3)
    tsdf[1, 1, 1] = 0.0                                                       # exactly 0: outside, no crossing
    assert tnp.extract(tsdf, np.ones_like(tsdf), (0, 0, 0), 1.0)[0].shape == (0, 3, 3)
    tsdf[1, 1, 1] = -0.5
    verts, _ = tnp.extract(tsdf, np.ones_like(tsdf), (0, 0, 0), 1.0)
    r = tnp.mesh_report(verts)
    assert len(verts) > 0 and (r.undirected == 2).all() and r.euler == 2 and r.volume > 0
    assert tnp.extract(np.ones((1, 4, 4), np.float32), np.ones((1, 4, 4), np.float32), (0, 0, 0), 1.0)[0].shape == (0, 3, 3)


# ---- the host build of the product's header ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("colors", (False, True))
def test_host_build_integrates_the_fusion_scene_byte_for_byte(colors):
    vol, views, images = tnp.fusion_scene()
    images = images if colors else None
    want, got, counters = tnp.empty_state(vol.dims, colors), tnp.empty_state(vol.dims, colors), {}
    tnp.integrate(want, vol, views, images, counters)
    outcomes = thc.integrate(got, vol, views, images)
    print(counters)
    # the scene reaches every outcome (measured on the restatement: 3437, 11586, 1939, 1837, 14368, 5233 and 6473)
    assert all(counters[name] >= 200 for name in tnp.OUTCOMES), counters
    assert sum(counters[name] for name in tnp.OUTCOMES[:6]) == 5 * 24 * 20 * 16
    assert outcomes.tolist() == [counters["behind"], counters["outside"], counters["unused"], counters["beyond_trunc"],
                                 counters["update_s_one"] + counters["update_s_below_one"]]
    assert got.tsdf.tobytes() == want.tsdf.tobytes() and got.weight.tobytes() == want.weight.tobytes()
    assert want.weight.max() == 2.0 and (want.weight == 0).any() and (want.weight == 1).any()
    if colors:
        assert got.rgb.tobytes() == want.rgb.tobytes() and want.rgb.any()
    # the fourth eye lies inside the volume: it alone has voxels behind it
    for k in range(5):
        c = {}
        tnp.integrate(tnp.empty_state(vol.dims), vol, views[k:k + 1], None, c)
        assert (c["behind"] > 0) == (k == 3)
    # any split of the list gives the same bytes
    split = tnp.empty_state(vol.dims, colors)
    thc.integrate(split, vol, views[:2], None if images is None else images[:2])
    thc.integrate(split, vol, views[2:], None if images is None else images[2:])
    assert split.tsdf.tobytes() == want.tsdf.tobytes() and split.weight.tobytes() == want.weight.tobytes()
    # the fused volume extracts to the same open mesh on both sides
    verts, cols = tnp.extract(want.tsdf, want.weight, vol.origin, vol.voxel_size, want.rgb)
    hv, hc, n = thc.extract(got.tsdf, got.weight, vol.origin, vol.voxel_size, got.rgb)
    assert n == len(verts) > 1000 and hv.tobytes() == verts.tobytes()
    assert set(tnp.mesh_report(verts).undirected.tolist()) == {1, 2}
    if colors:
        assert hc.tobytes() == cols.tobytes()


@pytest.mark.parametrize("colors", (False, True))
def test_host_build_extracts_the_sphere_byte_for_byte(colors):
    tsdf, weight, rgb, origin, voxel = tnp.sphere_volume(colors)
    verts, cols = tnp.extract(tsdf, weight, origin, voxel, rgb)
    hv, hc, n = thc.extract(tsdf, weight, origin, voxel, rgb)
    assert n == 2012 and hv.tobytes() == verts.tobytes()
    if colors:
        assert hc.tobytes() == cols.tobytes() and np.ptp(cols) > 0.5
    # capacity below the count: the rows that fit, the full count
    hv, _, n = thc.extract(tsdf, weight, origin, voxel, rgb, capacity=777)
    assert n == 2012 and hv.tobytes() == verts[:777].tobytes()


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sfgs.h")).read()
    lib = L.load()
    for name in ENTRY_POINTS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/sfgs.h"
        assert len(m.group(1).split(",")) == len(L.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    declared_version = int(re.search(r"#define SFGS_ABI_VERSION (\d+)", hdr).group(1))
    assert declared_version == L.ABI_VERSION == lib.sfgs_abi_version() == 28         # symbols were added, nothing else moved
    for struct, name in ((L.SfgsTsdfView, "SfgsTsdfView"), (L.SfgsTsdfVolume, "SfgsTsdfVolume")):
        fields = [f for f, _ in struct._fields_]
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        declared = [n for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                    for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
        assert declared == fields
        src = tmp_path / f"{name}.c"
        prints = "\n".join(f'  printf("{f} %zu\\n", offsetof({name}, {f}));' for f in fields)
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfgs.h"\nint main(void) {\n'
                       f'  printf("sizeof %zu\\n", sizeof({name}));\n{prints}\n  return 0;\n}}\n')
        exe = tmp_path / name
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
        assert int(out["sizeof"]) == C.sizeof(struct)
        for f in fields:
            assert int(out[f]) == getattr(struct, f).offset, f
    # a record is the consistency check's with an image pointer after the mask
    assert [f for f, _ in L.SfgsTsdfView._fields_ if f != "image"] == [f for f, _ in L.SfgsConsistencyView._fields_]


def test_the_library_refuses_bad_arguments_before_any_gpu_work():
    lib = L.load()
    dummy = C.c_double(0.0)
    fp = C.cast(C.byref(dummy), C.c_void_p).value        # never dereferenced: every call below is refused first

    def refused(rc, what):
        assert rc == E_ARG, what
        assert lib.sfgs_last_error(), what

    def table(n=3, image=None, **kw):
        t = (L.SfgsTsdfView * n)()
        for k in range(n):
            t[k] = L.SfgsTsdfView(fp, None, image, 8, 8, (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_double * 3)(), 4.0, 4.0, 10.0, 10.0)
        for name, v in kw.items():
            setattr(t[n - 1], name, v)
        return t

    assert lib.sfgs_tsdf_table_check(table(), 3, 0) == 0
    assert lib.sfgs_tsdf_table_check(table(1), 1, 0) == 0
    assert lib.sfgs_tsdf_table_check(table(256, image=fp), 256, 1) == 0
    for v in (0, -1, 257):
        refused(lib.sfgs_tsdf_table_check(table(), v, 0), v)
    refused(lib.sfgs_tsdf_table_check(None, 3, 0), "NULL table")
    refused(lib.sfgs_tsdf_table_check(table(), 3, 1), "no image for a volume with colours")
    refused(lib.sfgs_tsdf_table_check(table(image=fp), 3, 0), "an image for a volume without")
    for bad in ({"H": 0}, {"W": -1}, {"H": 1 << 16, "W": 1 << 15}, {"depth": None}, {"focal_x": 0.0}, {"focal_y": 0.0}):
        refused(lib.sfgs_tsdf_table_check(table(**bad), 3, 0), bad)
    assert b"SfgsTsdfView 2" in lib.sfgs_last_error()

    def volume(**kw):
        v = L.SfgsTsdfVolume(C.sizeof(L.SfgsTsdfVolume), 8, 8, 8, (C.c_double * 3)(), 0.5, 1.5, 64.0, fp, fp, None)
        for name, val in kw.items():
            setattr(v, name, val)
        return v

    bad_volumes = ({"struct_size": 8}, {"nx": 0}, {"ny": -3}, {"nz": 0}, {"nx": 1 << 11, "ny": 1 << 10, "nz": (1 << 9) + 1},
                   {"nx": 1 << 16, "ny": 1 << 16, "nz": 1}, {"voxel_size": 0.0}, {"voxel_size": float("inf")}, {"voxel_size": float("nan")},
                   {"trunc": 0.0}, {"trunc": -1.0}, {"trunc": float("nan")}, {"max_weight": 0.5}, {"max_weight": float("nan")},
                   {"tsdf": None}, {"weight": None}, {"origin": (C.c_double * 3)(0.0, float("nan"), 0.0)})
    for bad in bad_volumes:
        refused(lib.sfgs_tsdf_integrate(C.byref(volume(**bad)), fp, 3, None), bad)
        refused(lib.sfgs_tsdf_extract(C.byref(volume(**bad)), fp, None, 10, fp, fp, 1 << 20, None), bad)
    refused(lib.sfgs_tsdf_integrate(None, fp, 3, None), "volume")
    refused(lib.sfgs_tsdf_integrate(C.byref(volume()), None, 3, None), "table")
    for v in (0, 257):
        refused(lib.sfgs_tsdf_integrate(C.byref(volume()), fp, v, None), v)
    need = lib.sfgs_tsdf_scratch_bytes(8, 8, 8)
    assert need >= 8 * 3 and lib.sfgs_tsdf_scratch_bytes(1, 8, 8) > 0
    assert lib.sfgs_tsdf_scratch_bytes(0, 8, 8) == 0 and lib.sfgs_tsdf_scratch_bytes(1 << 11, 1 << 10, (1 << 9) + 1) == 0
    refused(lib.sfgs_tsdf_extract(C.byref(volume()), None, None, 10, fp, fp, need, None), "vertices")
    refused(lib.sfgs_tsdf_extract(C.byref(volume()), fp, None, 10, None, fp, need, None), "state")
    refused(lib.sfgs_tsdf_extract(C.byref(volume()), fp, None, 10, fp, None, need, None), "scratch")
    refused(lib.sfgs_tsdf_extract(C.byref(volume()), fp, None, -1, fp, fp, need, None), "capacity")
    refused(lib.sfgs_tsdf_extract(C.byref(volume()), fp, None, 10, fp, fp, need - 1, None), "scratch bytes")
    refused(lib.sfgs_tsdf_extract(C.byref(volume()), fp, fp, 10, fp, fp, need, None), "colors without rgb")
    refused(lib.sfgs_tsdf_extract(C.byref(volume(rgb=fp)), fp, None, 10, fp, fp, need, None), "rgb without colors")


def test_argument_checks_run_before_the_library_is_loaded(monkeypatch):
    from sfgs import tsdf as tm
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    assert set(tm.__all__) >= {"TsdfVolume", "TriangleSoup"} and not hasattr(tm, "install")
    ok = dict(origin=(0, 0, 0), dims=(4, 4, 4), voxel_size=0.5, trunc=1.5)
    for bad in ({"dims": (4, 4)}, {"dims": (4, 0, 4)}, {"dims": (4, 4.0, 4)}, {"dims": 4}, {"dims": (True, 4, 4)},
                {"dims": (1 << 11, 1 << 10, (1 << 9) + 1)}, {"trunc": 0.0}, {"trunc": -1.5}, {"trunc": np.nan}, {"trunc": np.inf},
                {"voxel_size": 0.0}, {"voxel_size": None}, {"max_weight": 0.5}, {"max_weight": np.nan}, {"max_weight": 0},
                {"origin": (0, 0)}, {"origin": (0, np.inf, 0)}, {"device": "cpu"}):
        with pytest.raises(ValueError):
            tm.TsdfVolume(**{**ok, **bad})
    # add_views on a volume that was never given device memory: every check below needs none
    cam = types.SimpleNamespace(R=np.eye(3), T=np.zeros(3), focal_x=100.0, focal_y=100.0)
    d, img = torch.ones(6, 8), torch.ones(3, 6, 8)

    def volume(colors):
        v = object.__new__(tm.TsdfVolume)
        v.dims, v.device, v._rgb = (4, 4, 4), torch.device("cuda:0"), (torch.zeros(3, 4, 4, 4) if colors else None)
        return v

    plain, coloured = volume(False), volume(True)
    with pytest.raises(ValueError, match="colors=True"):
        plain.add_views([d], [cam], images=[img])                             # images without colours
    with pytest.raises(ValueError, match="colors=True"):
        coloured.add_views([d], [cam])                                        # ... and the reverse
    with pytest.raises(ValueError, match="1 ... 256"):
        plain.add_views([d] * 257, [cam] * 257)
    with pytest.raises(ValueError, match="1 ... 256"):
        plain.add_views([], [])
    for depths, cams, masks in (([d, d], [cam], None), ([d, d], [cam, cam], [None]), (d, [cam], 5), ([d.double()], [cam], None),
                                ([torch.ones(2, 6, 8)], [cam], None), ([np.ones((6, 8), np.float32)], [cam], None),
                                ([d], [cam], [torch.ones(6, 8)]), ([d], [cam], [torch.ones(6, 7, dtype=torch.bool)]),
                                ([d], [types.SimpleNamespace(R=np.eye(3))], None),
                                ([d], [types.SimpleNamespace(**{**vars(cam), "focal_x": 0.0})], None)):
        with pytest.raises(ValueError):
            plain.add_views(depths, cams, masks)
    for images in ([img, img], [img.double()], [torch.ones(3, 6, 7)], [None]):
        with pytest.raises(ValueError):
            coloured.add_views([d], [cam], images=images)
    with pytest.raises(ValueError, match="GPU"):                              # everything else is right: the device check is last
        plain.add_views([d], [cam])
    with pytest.raises(ValueError, match="GPU"):
        coloured.add_view(d, cam, image=img)
    for capacity in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="capacity"):
            plain.extract(capacity)
    plain._tsdf = plain._weight = torch.zeros(4, 4, 4)
    for args in ((torch.zeros(4, 4, 3), torch.zeros(4, 4, 4)), (torch.zeros(4, 4, 4).double(), torch.zeros(4, 4, 4)),
                 (torch.zeros(4, 4, 4), torch.zeros(4, 4, 4), torch.zeros(3, 4, 4, 4))):
        with pytest.raises(ValueError):
            plain.load(*args)


# ---- PLY ---------------------------------------------------------------------------------------------------------------------------
def read_mesh_ply(path):
    """A reader of exactly what save_ply writes -> (header lines, vertex table, faces int32 [m,3])"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    np_of = {"float": "<f4", "double": "<f8", "uchar": "u1"}
    counts, fields, element = {}, [], None
    for line in lines[2:-1]:
        tok = line.split()
        if tok[0] == "element":
            element = tok[1]
            counts[element] = int(tok[2])
        elif element == "vertex":
            assert tok[0] == "property" and len(tok) == 3
            fields.append((tok[2], np_of[tok[1]]))
        else:
            assert line == "property list uchar int vertex_indices"
    assert list(counts) == ["vertex", "face"]
    vt = np.frombuffer(raw, dtype=np.dtype(fields), count=counts["vertex"], offset=end)
    ft = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=counts["face"], offset=end + vt.nbytes)
    assert end + vt.nbytes + ft.nbytes == len(raw) and (ft["n"] == 3).all()
    return lines, vt, ft["i"]


@pytest.mark.parametrize("colors", (False, True))
def test_save_ply_round_trips(tmp_path, colors):
    from sfgs.tsdf import TriangleSoup
    tsdf, weight, rgb, origin, voxel = tnp.sphere_volume(colors)
    verts, cols = tnp.extract(tsdf, weight, origin, voxel, rgb)
    n = len(verts)
    pad = lambda a: None if a is None else torch.from_numpy(np.concatenate([a, np.full((5, 3, 3), np.nan, np.float32)]))
    soup = TriangleSoup(pad(verts), pad(cols), torch.tensor([n]), n + 5)       # host tensors: weld and save_ply run on the host
    assert int(soup.num_triangles) == n and tuple(soup.vertices.shape) == (n, 3, 3)
    V, F = soup.weld()
    wantV, wantF = tnp.weld(verts)
    assert V.tobytes() == wantV.tobytes() and (F == wantF).all() and V.shape == (1008, 3) and F.shape == (n, 3)
    # welded, float
    lines, vt, faces = read_mesh_ply(_save(soup, tmp_path / "a.ply"))
    names = ["x", "y", "z"] + (["red", "green", "blue"] if colors else [])
    assert lines[2] == "element vertex 1008" and lines[3:3 + len(names)] == \
        [f"property {'float' if k < 3 else 'uchar'} {a}" for k, a in enumerate(names)]
    assert lines[3 + len(names)] == f"element face {n}"
    assert faces.min() == 0 and faces.max() == 1007 and (faces == F).all()
    assert np.stack([vt[a] for a in "xyz"], axis=1).tobytes() == V.tobytes()
    if colors:
        first = np.unique(verts.reshape(-1, 3).view(np.dtype((np.void, 12))).reshape(-1), return_index=True)[1]
        want = (cols.reshape(-1, 3)[first] * np.float32(255) + np.float32(0.5)).clip(0, 255).astype(np.uint8)
        assert (np.stack([vt[a] for a in ("red", "green", "blue")], axis=1) == want).all() and np.ptp(want) > 100
    # welded, double with an origin added in float64
    org = (512345.25, 3345678.5, 12.125)
    lines, vt, faces = read_mesh_ply(_save(soup, tmp_path / "sub" / "b.ply", origin=org))
    assert lines[3:6] == ["property double x", "property double y", "property double z"] and (faces == F).all()
    for j, a in enumerate("xyz"):
        assert vt[a].dtype == np.float64 and (vt[a] == V[:, j].astype(np.float64) + org[j]).all()
    # the soup as it is
    lines, vt, faces = read_mesh_ply(_save(soup, tmp_path / "c.ply", weld=False))
    assert lines[2] == f"element vertex {3 * n}" and (faces == np.arange(3 * n).reshape(-1, 3)).all()
    assert np.stack([vt[a] for a in "xyz"], axis=1).tobytes() == verts.tobytes()
    # sfgs.ply.read_ply still rejects list properties
    from sfgs.ply import read_ply
    with pytest.raises(NotImplementedError):
        read_ply(str(tmp_path / "a.ply"))
    # more found than stored: the views refuse
    short = TriangleSoup(pad(verts), pad(cols), torch.tensor([n + 6]), n + 5)
    with pytest.raises(ValueError, match="would have sufficed"):
        short.vertices


def _save(soup, path, **kw):
    soup.save_ply(str(path), **kw)
    return str(path)
