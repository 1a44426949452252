"""The other half of a kernel's contract: what the library writes BESIDES its outputs and what it reads that nobody wrote.
Every entry point that works in a caller-supplied scratch blob runs through its ordinary Python wrapper inside
tests/scratch_guard.py -- the blob between two guard bands, its body filled with 0x00, 0xFF and 0xA5 in turn -- and
  (a) no guard byte may change,
  (b) every output tensor and every returned counter must be the same BYTES as in the same call outside the harness, under
      every fill (every route here is documented bit-reproducible: no tolerance),
  (c) handed one byte less than it asked for, the library refuses (RuntimeError, its capacity message) before any launch:
      guards, the withheld byte and the whole body keep their fill, and an `out=` tensor keeps its sentinel.

FIRST WRITER of every scratch region, as read from the carve and the launch sequence of each entry (csrc/*.hip). "kernel" =
written by a kernel of the same call before any kernel reads it; nothing below is left to the previous call's bytes.
  fused_ssim            partials [tiles]: ssim_fwd, every tile; maps 3 x [B C H W] (train): ssim_fwd, every in-image pixel; the
                        backward reads in-image pixels only (halo outside the plane: masked to 0)
  loss                  coef[CF_*] (256-byte head): loss_final -- FIXED here: it wrote only the words of the route it ran and
                        loss_depth_bwd loads all seven (the unused ones never reach an output); now every word is written;
                        ssim / l1 partials [tiles]: loss_photo_fwd; depth partials [blocks][8]: loss_depth_fwd (7 of 8 words
                        written, 7 read); maps: loss_photo_fwd, as fused_ssim
  opacity entropy       partials [blocks] double: opacity_entropy_fwd, every block; the backward uses no scratch
  metrics (tile)        ssim / abs / sq partials [tiles]: metrics_tile, every tile
  metrics (stream)      partials [P * blocks][2] double: metrics_stream, every block
  depthvis              DvState + three histograms: ONE hipMemsetAsync over the whole blob (normalize=True; otherwise unused)
  dsmr register         pyramid levels u[k], v[k]: dsmr_downsample; part: dsmr_tile<1> before dsmr_mean reads it; mean: dsmr_mean
                        before dsmr_tile<2> / dsmr_select read it; level shifts / stats: dsmr_select of the level below
  dsm metrics           partials [5][blocks] double: dsm_metrics, every block
  pointcloud append     blk [blocks] uint64: pc_count, then scanned in place (the carry comes from the caller's state word)
  pointcloud bounds     part [6][blocks] double: pc_bounds, every block
  tsdf extract          blk [blocks] uint64: tsdf_count, then scanned in place
  mesh weld             table: hipMemsetAsync 0xff; slot_rep, flag: weld_insert / weld_rep, every soup vertex; the compaction's
                        plan: as compact
  mesh components       parent [m]: cc_init
  mesh clean            keep_vertex: hipMemsetAsync; keep_face: clean_mark, every face; two plans: as compact
  mesh decimate         table: hipMemsetAsync 0xff before each of its two uses; cells, bad: dec_cell; rep_of, flag: the key pass;
                        cluster_of: dec_sum, every vertex; first: dec_sum, by every cluster's representative (read for kept
                        clusters only); count, sums, color_sums, keep_cluster: ONE hipMemsetAsync; gfaces, keys, skip_face,
                        keep_face: dec_face, every face; face_rep: the second key pass (with drop_duplicates; not read
                        otherwise); three plans: as compact
  mesh vertex_faces     cursor [m]: hipMemsetAsync; block_sum: vf_chunk_sum. vertex_normals uses no scratch
  mesh render           list_count + count_lines: hipMemsetAsync 0; keys: hipMemsetAsync 0xff; rec [m]: mr_project; list_large /
                        list_huge: mr_face (entries below list_count only are read)
  simple_knn (spatial)  count [M]: hipMemsetAsync; bounds: knn_bounds; keys: knn_count; block_sum: knn_scan_sums; start:
                        knn_scan_apply; sorted: knn_scatter; blo / bhi, slo / shi: knn_boxes
  filter3d              dist [N], block_max [blocks]: filter3d_min_depth
  compact               total: scan_sums (hipMemsetAsync when N = 0); block_sum: compact_count; dst_index [N]: compact_index
  select_kth            SelectState (k, prefix, mask, mult, succ, hist[2048]): select_init; hist cleared again by every pick
  densify               code [N], block_sum [blocks][5]: densify_decide; totals: scan_sums; idx [N][4]: densify_index
  rasterizer forward    tiles blob: header, duplicate pools, coarse counters by zero_head_kernel; tile_range (every tile of every
                        coarse bin, empty ones as (0, 0)), long_tiles (HDR_LONG_COUNT entries), block_nvis / block_dref, sc_cnt /
                        sc_hits / sc_base, tile_order (when ordered) by the plan / sort kernels. geom: rec and dup by preprocess
                        (dup of a huge splat by big_walk), read only for radii > 0 / through the lists; big_list, block_items by
                        preprocess. bins: pairs by preprocess, csr / slabs by the binning, items / sorted_id / sorted_dup by the
                        sorts (slots of a list's alignment padding are never read). image: n_contrib / final_T / dacc per in-image
                        pixel, tile_kmax / tile_dead per tile, hitmask per 64-entry group up to the last contributor's, all by
                        composite_fwd; the backward starts at tile_kmax and returns before any hitmask read when it is 0
  rasterizer backward   dupgrad: records by composite_bwd (zero records for dead entries, or the live flags + zero line by
                        dupgrad_prefill); FIXED here: with no duplicates the 256-byte dummy of the wrapper was written far behind
                        its end under prefill=always (below: test_zero_duplicate_frame)
Unreachable through the wrappers: a backward over a band-rendered frame (tile_kmax / tile_dead of the tiles outside the band
stay unwritten; diff_gauss refuses tile_rows with a backward); short rasterizer scratch (diff_gauss passes the size it computed,
not the tensor's); BlendStats.add takes its blobs from sfgs.shard, outside the two allocation sites (its bytes are compared).
"""
import functools
import types

import numpy as np
import pytest
import torch

from scratch_guard import GUARD, ScratchGuard

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILLS = (0x00, 0xFF, 0xA5)
REFUSAL = r"too small|bytes given"          # the library's capacity messages


# ---- the three steps -----------------------------------------------------------------------------------------------------------------
def snapshot(value, name="out", into=None):
    """Every tensor / array / number of a (nested) result as bytes, keyed by its path."""
    into = {} if into is None else into
    if isinstance(value, torch.Tensor):
        a = value.detach().cpu().contiguous()
        into[name] = (str(a.dtype), tuple(a.shape), a.reshape(-1).view(torch.uint8).numpy().tobytes() if a.numel() else b"")
    elif isinstance(value, np.ndarray):
        into[name] = (str(value.dtype), value.shape, np.ascontiguousarray(value).tobytes())
    elif isinstance(value, dict):
        for k, v in value.items():
            snapshot(v, f"{name}.{k}", into)
    elif isinstance(value, (tuple, list)):
        for k, v in enumerate(value):
            snapshot(v, f"{name}[{k}]", into)
    else:
        assert value is None or isinstance(value, (int, float, bool, str, np.integer, np.floating)), (name, type(value))
        into[name] = repr(value)
    return into


def assert_same(want, got, what):
    assert sorted(want) == sorted(got), (what, sorted(want), sorted(got))
    for k in want:
        if want[k] != got[k]:
            if isinstance(want[k], tuple) and want[k][:2] == got[k][:2]:
                a, b = np.frombuffer(want[k][2], np.uint8), np.frombuffer(got[k][2], np.uint8)
                bad = np.flatnonzero(a != b)
                raise AssertionError(f"{what}: {k} {want[k][:2]} differs in {bad.size} bytes, first at byte {int(bad[0])}")
            raise AssertionError(f"{what}: {k} differs: {str(want[k])[:200]} != {str(got[k])[:200]}")


def contract(monkeypatch, run, scratch_expected=True, **guard_kw):
    """(a) the wrapper inside the harness, (b) check(), (c) bytes equal to the call outside the harness -- under every fill."""
    want = snapshot(run())
    assert_same(want, snapshot(run()), "outside the harness, run twice")       # the premise: bit-reproducible
    for fill in FILLS:
        with ScratchGuard(monkeypatch, fill=fill, device=DEV, **guard_kw) as sg:
            got = snapshot(run())
            sg.check()
            assert bool(sg.handed) == scratch_expected, [h.entry for h in sg.handed]
        assert_same(want, got, f"fill 0x{fill:02X}")
    return sg


def refused(monkeypatch, run, short_for=None, untouched=()):
    """(c) of the module text. untouched: [(tensor, byte)] -- `out=` tensors that must keep their sentinel."""
    with ScratchGuard(monkeypatch, fill=0x5A, device=DEV, short=1, short_for=short_for) as sg:
        with pytest.raises(RuntimeError, match=REFUSAL):
            run()
        sg.check()
        assert sg.short_tails_intact() and sg.shortened_bodies_intact(), [(h.entry, h.asked) for h in sg.handed]
    for t, byte in untouched:
        assert bool((t.reshape(-1).view(torch.uint8) == byte).all())


def dev(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, order="C"))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---- fused_ssim, loss, opacity entropy, metrics, depthvis ------------------------------------------------------------------------------
def ssim_run(shape):
    g = torch.Generator().manual_seed(shape[2] * 1000 + shape[3])          # the pair of tests/test_gpu_ops.py's tile-boundary test
    a = torch.rand(*shape, generator=g)
    b = (a + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1).to(DEV)
    a = a.to(DEV)

    def run():
        from fused_ssim import fused_ssim
        x = a.clone().requires_grad_(True)
        v = fused_ssim(x, b)
        (0.2 * (1.0 - v)).backward()
        return dict(value=v, grad=x.grad, no_grad=fused_ssim(a, b, train=False))
    return run


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 45, 65)])
def test_fused_ssim(monkeypatch, shape):
    contract(monkeypatch, ssim_run(shape))


def loss_run(shape, kind="training"):
    from test_gpu_loss import depth_pair, image_pair, make_mask
    c, h, w = shape
    a, b = (dev(t) for t in image_pair(c, h, w, h * 1000 + w))
    gt_depth, depth = (dev(t) for t in depth_pair(h, w, h * 1000 + w))
    mask = dev(make_mask("fractional", h, w, h * 1000 + w))

    def run():
        from sfgs import loss
        x, d = a.clone().requires_grad_(True), depth.clone().requires_grad_(True)
        if kind == "training":
            total, Ll1, ssim, depth_loss = loss.training_loss(x, d, b, gt_depth, mask, 0.2, 0.05)
            total.backward()                                              # the forward's scratch again: one entry, checked after it
            return dict(loss=total, Ll1=Ll1, ssim=ssim, depth_loss=depth_loss, g_image=x.grad, g_depth=d.grad)
        value = loss.l1_loss(x, b)                                        # the streaming L1: the other route of the coefficients
        value.backward()
        return dict(value=value, grad=x.grad)
    return run


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 45, 65), (1, 67, 130)])
def test_training_loss_with_mask_and_depth_pair(monkeypatch, shape):
    contract(monkeypatch, loss_run(shape))


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 45, 65)])
def test_l1_stream_loss(monkeypatch, shape):
    contract(monkeypatch, loss_run(shape, "l1"))


def entropy_run(n, dtype):
    from test_gpu_opacity_reg import DTYPES, fused, raw_opacities
    x = raw_opacities(n, DTYPES[dtype], n).to(DEV)
    return lambda: fused(x)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2049])                  # 2049: a third workgroup of 4 x 256 floats, a fifth of 2 x 256 doubles
def test_opacity_entropy(monkeypatch, n, dtype):
    contract(monkeypatch, entropy_run(n, dtype))


def metrics_run(shape, ssim, out=None):
    from test_gpu_metrics import pair
    a, b = (dev(t) for t in pair(shape))

    def run():
        from sfgs import metrics
        rows = [metrics.view_metrics(a, b, clamp=clamp, ssim=ssim, out=out) for clamp in (True, False)]
        return rows[-1] if out is not None else rows
    return run


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 45, 65)])
def test_metrics_tile_route(monkeypatch, shape):
    contract(monkeypatch, metrics_run(shape, True))


@pytest.mark.parametrize("shape", [(4, 1, 1), (3, 7, 5), (1, 300, 301)])       # pixels; odd; several blocks per plane, ragged
def test_metrics_stream_route(monkeypatch, shape):
    contract(monkeypatch, metrics_run(shape, False))


def depthvis_run(H, W):
    import depthvis_np as dnp
    d = dev(dnp.make_depth("uniform" if H * W < 100 else "special", H, W, 31))
    m = dev(dnp.make_mask(H, W, 31))

    def run():
        from sfgs import depthvis
        return dict(f=depthvis.colorize_depth(d[None], m[None], normalize=True, out="float_chw"),
                    u=depthvis.colorize_depth(d, None, normalize=True, out="uint8_hwc"))
    return run


@pytest.mark.parametrize("H,W", [(1, 1), (37, 53), (67, 130)])                  # 67 x 130: a third histogram workgroup
def test_depthvis(monkeypatch, H, W):
    contract(monkeypatch, depthvis_run(H, W))


# ---- geometry, pointcloud, tsdf ----------------------------------------------------------------------------------------------------
def register_run(which):
    import geometry_np as gnp
    if which == "1x1":
        ref = sec = np.array([[3.0]])
    else:                                                 # test_gpu_geometry's fresh pair: two shapes, a pyramid, infinities
        ref, sec = gnp.shifted_pair(103, 131, 21, -3, 6, 0.5, sec_shape=(90, 140))
        ref.reshape(-1)[[4, 44, 444]] = [np.inf, -np.inf, np.inf]
    r, s = dev(ref), dev(sec)

    def run():
        from sfgs.geometry import register
        out = register(r, s, irange=5, scaling=True)
        return dict(shift=out.shift, ab=out.ab, stats=out.stats)
    return run


@pytest.mark.parametrize("which", ["1x1", "103x131"])
def test_dsmr_register(monkeypatch, which):
    contract(monkeypatch, register_run(which))


def dsm_metrics_run(which):
    import geometry_np as gnp
    pred, gt = (np.array([[3.0]]), np.array([[2.5]])) if which == "1x1" else gnp.shifted_pair(300, 517, 8, 0, 0, 0.4)
    p, g = dev(pred), dev(gt)
    keep = dev(np.random.default_rng(3).random(pred.shape) < 0.8)

    def run():
        from sfgs.geometry import dsm_metrics
        return [dsm_metrics(p, g), dsm_metrics(p, g, mask=keep)]
    return run


@pytest.mark.parametrize("which", ["1x1", "300x517"])                           # 300 x 517: more than one workgroup per partial
def test_dsm_metrics(monkeypatch, which):
    contract(monkeypatch, dsm_metrics_run(which))


def pointcloud_run(case, colors=False):
    from test_gpu_pointcloud import BOUNDARY_CASES, CAM, seeded_depth
    H, W, mask = BOUNDARY_CASES[case]
    lead, depth = dev(seeded_depth(3, 5, 1)), dev(seeded_depth(H, W, H * 1000 + W))
    mask = None if mask is None else dev(mask)
    images = [dev(np.random.default_rng(k).random((3,) + s, dtype=np.float32)) for k, s in enumerate(((3, 5), (H, W)))] if colors else [None] * 2

    def run():
        from sfgs.pointcloud import PointCloud
        pc = PointCloud(15 + H * W, colors=colors, device=DEV)
        pc.add_view(lead, CAM, image=images[0])                              # the case starts at a carried row
        pc.add_view(depth, CAM, mask=mask, image=images[1])
        points, cols = pc.result()
        return dict(n=pc.num_points, points=points, colors=cols, bounds=pc.bounds())
    return run


@pytest.mark.parametrize("case,colors", [("1x1_used", False), ("half_random", True), ("more_workgroups_than_one_scan_round", False)])
def test_pointcloud_append_and_bounds(monkeypatch, case, colors):
    contract(monkeypatch, pointcloud_run(case, colors))


def loaded_volume(case):
    from sfgs.tsdf import TsdfVolume
    tsdf, weight, rgb, origin, voxel = case
    nz, ny, nx = tsdf.shape
    v = TsdfVolume(origin, (nx, ny, nz), voxel, trunc=1.0, colors=rgb is not None, device=DEV)
    return v.load(dev(tsdf), dev(weight), None if rgb is None else dev(rgb))


def tsdf_run(which):
    import tsdf_np as tnp
    # wavy: 71 x 63 x 63 cells = more than 1024 workgroups of 256: the scan's second round (152 114 triangles: tests/test_gpu_mesh.py)
    v, capacity = (loaded_volume(tnp.sphere_volume(True)), 2012) if which == "sphere" else (loaded_volume(tnp.wavy_volume((72, 64, 64), colors=True)), 152114)

    def run():
        soup = v.extract(capacity)
        return dict(n=soup.num_triangles, vertices=soup.vertices, colors=soup.colors)
    return run


@pytest.mark.parametrize("which", ["sphere", "wavy"])
def test_tsdf_extract(monkeypatch, which):
    contract(monkeypatch, tsdf_run(which))


# ---- mesh ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup_of(which):
    """-> (soup vertices [n,3,3], colours) on the device: one triangle, or the islands (17 338 triangles, 8 704 welded vertices: a
    third 4 096-row chunk of the compaction plans, 34 workgroups of 256)"""
    if which == "triangle":
        tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
        return dev(tri), dev(tri * 0.5)
    import mesh_np as mnp
    soup = loaded_volume(mnp.islands_volume()).extract(20000)
    assert int(soup.num_triangles) == 17338
    return soup.vertices.contiguous(), soup.colors.contiguous()


@functools.lru_cache(maxsize=None)
def mesh_of(which):
    from sfgs.mesh import weld
    return weld(*soup_of(which))


def mesh_fields(mesh):
    return dict(m=mesh.num_vertices, n=mesh.num_faces, V=mesh.vertices, F=mesh.faces, C=mesh.colors)


def mesh_run(op, which):
    from sfgs.mesh import weld
    if op == "weld":
        soup = soup_of(which)
        return lambda: mesh_fields(weld(*soup))
    mesh = mesh_of(which)
    if op == "components":
        def run():
            cc = mesh.components()
            return dict(labels=cc.labels, triangles=cc.triangles, vertices_in=cc.vertices_in, count=cc.count, checked=cc.check())
    elif op == "clean":
        run = lambda: [mesh_fields(mesh.clean(min_triangles=25)), mesh_fields(mesh.clean(largest=1, drop_degenerate=True))]
    elif op == "decimate":
        def run():
            out = []
            for drop in (True, False):
                dec, vmap = mesh.decimate(0.75, origin=(0.13, -0.2, 0.31), drop_duplicates=drop, return_map=True)
                out.append(dict(mesh_fields(dec), vmap=vmap))
            return out
    elif op == "vertex_faces_and_normals":
        def run():
            adj = mesh.vertex_faces()
            normals = mesh.vertex_normals(adj)
            return dict(offsets=adj.offsets, records=adj.records, normals=normals, status=adj.check())
    else:
        import mesh_render_np as mr
        normals = mesh.vertex_normals()
        cam = mr.islands_orbit_camera()

        def run():
            out = []
            for kw in (dict(), dict(cull="back", normals=normals), dict(_small_max=0)):      # _small_max=0: every face through the lists
                view = mesh.render(cam, 40, 48, **kw)
                out.append(dict(depth=view.depth, face=view.face, normal=view.normal, rgb=view.rgb, counts=view.counts, checked=view.check()))
            return out
    return run


@pytest.mark.parametrize("which", ["triangle", "islands"])
@pytest.mark.parametrize("op", ["weld", "components", "clean", "decimate", "vertex_faces_and_normals", "render"])
def test_mesh(monkeypatch, op, which):
    contract(monkeypatch, mesh_run(op, which))


# ---- model-side kernels: kNN, 3D filter, compaction, densification ---------------------------------------------------------------------
def knn_run(n):
    from test_gpu_knn_spatial import _cloud
    pts = dev(_cloud("uniform", n, seed=n % 97))

    def run():
        from simple_knn._C import distCUDA2
        return distCUDA2(pts)
    return run


@pytest.mark.parametrize("n", [32769, 40000])                                   # 32 769: the first cloud of the spatial path
def test_knn_spatial_path(monkeypatch, n):
    contract(monkeypatch, knn_run(n))


def filter3d_run(n):
    from model_ops_ref import camera
    rng = np.random.default_rng(n)
    xyz = dev(np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.uniform(1, 9, (n, 1))], 1).astype(np.float32))
    cams = [types.SimpleNamespace(**camera()), types.SimpleNamespace(**camera(T=(0.5, -0.2, 1.0), focal=900.0, W=320, H=200, cx=0.02))]

    def run():
        from sfgs.filter3d import compute_3D_filter
        return compute_3D_filter(xyz, cams)
    return run


@pytest.mark.parametrize("n", [1, 2049])                                        # 2049: a ninth workgroup, one point in it
def test_filter3d(monkeypatch, n):
    contract(monkeypatch, filter3d_run(n))


def compact_run(n):
    rng = np.random.default_rng(n)
    keep = dev(rng.random(n) < 0.6)
    keep[-1] = True
    ts = [dev(rng.random((n, 3), dtype=np.float32)), dev(rng.integers(0, 1 << 40, (n,))), dev(rng.random((n, 15, 3), dtype=np.float32)),
          dev(rng.integers(0, 255, (n, 3), dtype=np.uint8))]

    def run():
        from sfgs.compact import compact_rows
        return compact_rows(keep, ts)                      # plan and rows: the rows read the plan's scratch
    return run


@pytest.mark.parametrize("n", [1, 2049, 4097])                                  # 4097: a second workgroup of 256 x 16 rows
def test_compact_plan_and_rows(monkeypatch, n):
    contract(monkeypatch, compact_run(n))


def select_run(n):
    from test_gpu_densify_edges import _values
    v = dev(_values("random_bits", n).view(np.float32))    # zeros, denormals, the whole exponent range, +inf, duplicates

    def run():
        from sfgs.densify import quantile_linear
        return [quantile_linear(v, q) for q in (0.0, 0.37, 1.0)]
    return run


@pytest.mark.parametrize("n", [1, 4097])                                        # 4097: a second workgroup of 256 x 16 values
def test_select_kth(monkeypatch, n):
    contract(monkeypatch, select_run(n))


def densify_run(n, what):
    import densify_ref as DR
    from test_gpu_densify_edges import ATTR, GROUPS, STATS, _Model, _inputs, _model
    inp = _inputs(n)
    c = inp.cfg
    if what == "masks":
        m = _Model(_xyz=dev(inp.params["xyz"]), _scaling=dev(inp.params["scaling"]), _opacity=dev(inp.params["opacity"]),
                   xyz_gradient_accum=dev(inp.xyz_gradient_accum), xyz_gradient_accum_abs=dev(inp.xyz_gradient_accum_abs),
                   denom=dev(inp.denom), percent_dense=c["percent_dense"])

        def run():
            from sfgs import densify
            return densify.decide_masks(m, inp.max_grad, c["min_opacity"], c["extent"], 20)     # decide + masks
        return run
    _, samples, moments = DR.reference(inp, 20, moments=DR.moments_for(inp, "some"))

    def run():
        from sfgs import densify
        m = _model(inp, moments, torch.device(DEV))        # the surgery replaces the model's tensors: a fresh one per run
        ret = densify.densify_and_prune(m, inp.max_grad, c["min_opacity"], c["extent"], 20, samples=samples.clone())     # decide, gather, children
        out = dict(ret=[int(v) for v in ret])
        for name in GROUPS:
            p = getattr(m, ATTR[name])
            st = m.optimizer.state.get(p) or {}
            out[name] = dict(p=p, exp_avg=st.get("exp_avg"), exp_avg_sq=st.get("exp_avg_sq"))
        for k in STATS + ("max_radii2D",):
            out[k] = getattr(m, k)
        return out
    return run


@pytest.mark.parametrize("what", ["masks", "surgery"])
@pytest.mark.parametrize("n", [1, 2049])                                        # 2049: a ninth workgroup, one row in it
def test_densify(monkeypatch, n, what):
    contract(monkeypatch, densify_run(n, what))


# ---- the rasterizer ----------------------------------------------------------------------------------------------------------------
RASTER_CASES = ("precomp_small", "sh1_ragged", "big_splats", "lists_2k")


@functools.lru_cache(maxsize=None)
def raster_inputs(case):
    from sfgs.synth import scene, upstream_grads
    from test_gpu_raster import CASES
    c = CASES[case]
    frame, g = scene(c["n"], c["W"], c["H"], seed=c.get("seed", 7), **c["kw"])
    gc, gd = upstream_grads(c["W"], c["H"], 0)
    return frame, g, gc, gd


def forget_earlier_frames():
    """Every run starts where a process starts: no launch hints, no capacities learnt -- the first frame launches everything, the
    second runs under the hints the first one taught. The runs inside and outside the harness then take the same routes."""
    import diff_gauss
    torch.cuda.synchronize()
    diff_gauss._hint_state.clear()
    diff_gauss._cap_hint.clear()


def raster_run(case, frames=2):
    from test_gpu_raster import run_hip
    frame, g, gc, gd = raster_inputs(case)

    def run():
        forget_earlier_frames()
        return [run_hip(frame, g, gc, gd) for _ in range(frames)]              # images, radii, counters, every gradient
    return run


# What the WRAPPER planned with is not a counter of the frame: a first frame whose plan overflows (sh1_ragged: more duplicates
# than 4 N) is planned again from the overflowing attempt's counts, and in such an attempt WHICH preprocess workgroups still got
# duplicate indices from the pools -- and so how many items the fullest slab saw -- is decided by the order of their atomics
# (seen: coarse_capacity 474 against 472 between two runs). The attempt that fits, the only one whose results are returned, does
# not depend on it.
PLANNED_WITH = ("dup_capacity", "coarse_capacity", "plan_attempts")


def strip(outs):
    outs = [{k: v for k, v in o.items() if k not in ("norm", "extra")} for o in outs]
    for o in outs:
        o["counters"] = {k: v for k, v in o["counters"].items() if k not in PLANNED_WITH}
    return outs


@pytest.mark.parametrize("case", RASTER_CASES)
def test_rasterizer_two_frames(monkeypatch, case):
    run = raster_run(case)
    sg = contract(monkeypatch, lambda: strip(run()))
    assert sorted({h.entry for h in sg.handed}) == ["diff_gauss.backward", "diff_gauss.forward"]
    if case == "precomp_small":                            # (no huge splat in it: the first frame teaches NO_HUGE_SPLATS at least)
        second = run()[1]["counters"]
        assert second["fwd_hints"] != 0, second            # the second frame did run under launch hints


@pytest.mark.parametrize("option", [("sort", "split"), ("binning", "direct"), ("prefill", "always"), ("prefill", "never")],
                         ids=lambda o: "=".join(o))
@pytest.mark.parametrize("case", ["precomp_small", "big_splats"])
def test_rasterizer_routes(monkeypatch, sfgs_option, case, option):
    run = raster_run(case)
    default = strip(run())
    sfgs_option(*option)
    contract(monkeypatch, lambda: strip(run()))
    routed = strip(run())
    for a, b in zip(default, routed):                                           # every route: the same images and gradients
        assert_same(snapshot({k: a[k] for k in ("color", "depth", "alpha", "radii", "grads")}),
                    snapshot({k: b[k] for k in ("color", "depth", "alpha", "radii", "grads")}), f"{option} against the default route")


def test_blend_stats_add(monkeypatch):
    from test_gpu_importance import _inputs, _settings
    frame, g, _, _ = raster_inputs("precomp_small")
    t, settings = _inputs(g), _settings(frame)

    def run():
        from sfgs.importance import BlendStats
        forget_earlier_frames()
        s = BlendStats(t["means3D"].shape[0], torch.device(DEV))
        views = [s.add(settings, **t) for _ in range(2)]
        return dict(views=views, q=s.weight_sum_q32, max=s.weight_max, hits=s.hits, seen=s.views)
    contract(monkeypatch, run, scratch_expected=False)     # its blobs come from sfgs.shard: bytes only (module text)


@pytest.mark.parametrize("prefill", ["auto", "always", "never"])
def test_zero_duplicate_frame(monkeypatch, sfgs_option, prefill):
    """16 Gaussians behind the camera at 64 x 48, with a backward: the wrapper hands the library a 256-byte dupgrad dummy. Until
    this test the prefill kernel stored its 256-byte zero line at dupgrad + dupgrad_zero_offset(capacity) under prefill=always --
    for this frame's capacity of 4 416 list slots that is byte 216 576, far beyond a 64 KiB guard: the guard of this test is
    sized from the frame's own dupgrad_bytes so that the store would have landed inside it."""
    import diff_gauss
    from sfgs import _lib as L
    from sfgs.synth import scene, upstream_grads
    from test_gpu_raster import run_hip
    frame, g = scene(16, 64, 48, seed=1, zrange=(4., 8.), scale_range=(0.01, 0.2))
    behind = dict(g, means3D=g["means3D"] * torch.tensor([1., 1., -1.]))
    gc, gd = upstream_grads(64, 48, 0)
    lib = L.load()
    over = diff_gauss._layout(lib, 16, 64, 48, 0, 0, False)[2]
    cap = 4 * 16 + over                                                        # what the wrapper plans a first frame of 16 with
    dupgrad_bytes = diff_gauss._layout(lib, 16, 64, 48, cap, 256, True)[1]
    guard = -(-(dupgrad_bytes + 256) // 512) * 512
    assert (cap, dupgrad_bytes - 256) == (4416, 216576) and dupgrad_bytes - 256 > GUARD and guard >= dupgrad_bytes
    ordinary = raster_run("precomp_small", frames=1)
    want = strip(ordinary())
    sfgs_option("prefill", prefill)
    for fill in FILLS:
        forget_earlier_frames()
        with ScratchGuard(monkeypatch, fill=fill, device=DEV, guard=guard) as sg:
            out = run_hip(frame, behind, gc, gd * 0)
            sg.check()
            dummy = [h for h in sg.handed if h.entry == "diff_gauss.backward"]
            assert [h.asked for h in dummy] == [256] and out["counters"]["dup_capacity"] == cap and out["counters"]["num_duplicates"] == 0
        assert np.all(out["radii"] == 0) and np.all(out["alpha"] == 0)
        for k, v in out["grads"].items():
            assert v.tobytes() == np.zeros_like(v).tobytes(), (k, fill)        # every gradient is (+)zero
        got = strip(ordinary())                                                # a following ordinary frame on the same stream
        for k in ("color", "depth", "alpha", "radii", "grads"):
            assert_same(snapshot(want[0][k]), snapshot(got[0][k]), f"the ordinary frame after the empty one: {k}, fill 0x{fill:02X}")


# ---- short scratch -----------------------------------------------------------------------------------------------------------------
def refused_out_row():
    row = torch.full((8,), float("nan"), dtype=torch.float64, device=DEV)
    row.view(torch.uint8).fill_(0xC7)
    return row


SHORT = {
    "fused_ssim": lambda: (ssim_run((2, 3, 45, 65)), None),
    "training_loss": lambda: (loss_run((3, 45, 65)), None),
    "l1_stream_loss": lambda: (loss_run((3, 45, 65), "l1"), None),
    "opacity_entropy": lambda: (entropy_run(2049, "f32"), None),
    "depthvis": lambda: (depthvis_run(37, 53), None),
    "dsmr_register": lambda: (register_run("103x131"), None),
    "dsm_metrics": lambda: (dsm_metrics_run("300x517"), None),
    "pointcloud_append": lambda: (pointcloud_run("half_random"), "add_depth"),
    "pointcloud_bounds": lambda: (pointcloud_run("half_random"), "bounds"),
    "tsdf_extract": lambda: (tsdf_run("sphere"), None),
    "mesh_weld": lambda: (mesh_run("weld", "islands"), None),
    "mesh_components": lambda: (mesh_run("components", "islands"), None),
    "mesh_clean": lambda: (mesh_run("clean", "islands"), "sfgs.mesh.clean"),
    "mesh_decimate": lambda: (mesh_run("decimate", "islands"), None),
    "mesh_vertex_faces": lambda: (mesh_run("vertex_faces_and_normals", "islands"), None),
    "knn_spatial": lambda: (knn_run(32769), None),
    "filter3d": lambda: (filter3d_run(2049), None),
    "compact_plan": lambda: (compact_run(2049), None),
    "select_kth": lambda: (select_run(4097), None),
    "densify_decide": lambda: (densify_run(2049, "masks"), "sfgs.densify._decide"),
}


@pytest.mark.parametrize("entry", sorted(SHORT))
def test_short_scratch_is_refused(monkeypatch, entry):
    run, short_for = SHORT[entry]()
    refused(monkeypatch, run, short_for)


@pytest.mark.parametrize("ssim", [True, False], ids=["tile", "stream"])
def test_short_scratch_is_refused_metrics_and_its_row_untouched(monkeypatch, ssim):
    row = refused_out_row()
    refused(monkeypatch, metrics_run((3, 45, 65), ssim, out=row), untouched=[(row, 0xC7)])


def test_short_scratch_is_refused_mesh_render_and_its_view_untouched(monkeypatch):
    import mesh_render_np as mr
    mesh, cam = mesh_of("islands"), mr.islands_orbit_camera()
    view = mesh.render(cam, 40, 48)
    planes = [view.depth, view.face, view.normal, view.rgb, view._state]
    for t in planes:
        t.view(torch.uint8).fill_(0xC7)
    refused(monkeypatch, lambda: mesh.render(cam, 40, 48, out=view), untouched=[(t, 0xC7) for t in planes])
