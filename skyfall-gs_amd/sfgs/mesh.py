"""sfgs.mesh -- the triangle soup of sfgs.tsdf finished on the device (csrc/mesh.hip through libsfgs.so): welded into an indexed
mesh, its connected components labelled and counted, floaters and degenerate faces removed. The reference has no mesh step.

    soup = vol.extract(capacity=8_000_000)                             # sfgs.tsdf
    mesh = soup.mesh()                                                 # weld: V [m,3], F [n,3] int32, colours; nothing read back
    cc = mesh.components()                                             # labels [m], triangles [m], vertices_in [m], count
    clean = mesh.clean(min_triangles=64, largest=1)                    # a new Mesh; drop_degenerate=True drops zero-area faces
    clean.save_ply("city.ply", origin=(utm_x, utm_y, alt))

Weld (include/sfgs.h states it in full, tests/mesh_np.py in numpy; the kernels equal that restatement byte for byte): two soup
vertices are one when their twelve bytes are equal (-0.0 is not +0.0, NaNs are equal when their bits are); the unique vertices
are numbered in order of first appearance and take the colour of that first appearance. Sorting V by its bytes gives
TriangleSoup.weld()'s V. Components: every face joins its three indices, a label is the smallest vertex index of the component,
`triangles` counts the faces by their first index (degenerate faces too). Clean keeps a component when it has at least
min_triangles faces and is among the first `largest` ordered by (triangles descending, label ascending); a face when its
component is kept and, with drop_degenerate, its three indices differ; a vertex when a kept face references it. Order is preserved.

A Mesh's buffers are sized for the worst case and its counts live on the device; the sized views (vertices, faces, colors) cost
ONE host read per Mesh, on first use, which also reports a status the kernels left (an index out of range, a loop bound reached).
components() and clean() need their input's sizes and so count as such a use; what they return is read back only when asked.

Decimate, adjacency, normals (include/sfgs.h in words, tests/mesh_simplify_np.py in numpy; byte for byte as well):

    small = clean.decimate(cell=2 * voxel, origin=vol_origin)          # vertex clustering: a new Mesh at most as large
    adj = small.vertex_faces()                                         # (offsets [m+1], records [3n]): corner records 3t+c per vertex
    normals = small.vertex_normals(adjacency=adj)                      # float32 [m,3], area-weighted, summed in a fixed order
    small.save_ply("city_small.ply", origin=(utm_x, utm_y, alt), normals=normals)

decimate puts every vertex into the cell floor((x - origin) / cell) of a grid, replaces each cell's vertices by their mean (an
integer mean of 32-bit fixed-point offsets inside the cell, so it does not depend on the order of summation; a cell with one
vertex keeps that vertex's bytes), maps the faces through the cells and drops those that collapse, those that repeat an earlier
face's set of three vertices (drop_duplicates) and then every cell no face is left on. A vertex whose cell is not finite or
leaves int32 is bad: it joins no cell, its faces go, and the result's first sized use raises ValueError.

Render (csrc/mesh_raster.hip; include/sfgs.h in words, tests/mesh_render_np.py in numpy; byte for byte as well):

    view = small.render(camera, 1024, 1024, normals=normals, cull="back")   # MeshView: depth [1,H,W], face [H,W], normal, rgb
    drawn, culled, clipped, degenerate = view.check()                       # ONE host read

Every vertex is projected in float64 and snapped to 1/256 pixel; coverage is decided by int64 edge functions with a top-left
rule (a pixel centre on an edge two faces share belongs to exactly one of them), depth is interpolated perspective-correctly
and rounded to float32, and a pixel goes to the smallest (depth bits, face index): no order of arrival changes a byte. The
rendered depth is an ordinary view, as a ray-cast one is: it goes into add_views, evaluate_dsm, sfgs.pointcloud, sfgs.ortho
and ViewSet. There is NO near-plane clipping: a face with a vertex at or in front of `near` (or beyond 2^20 pixels from the
image's origin, or not finite) is not drawn as a whole and counted as clipped -- keep the camera outside the mesh's
triangles, or expect holes where they cross the camera's plane. No anti-aliasing, no textures.

There is no hole filling or smoothing, and no torch fallback: without the HIP library every operator raises."""
import math
import os

import numpy as np
import torch

from . import _call
from . import _lib as L
from .geometry import _check_view, _vec
from .tsdf import _positive

__all__ = ["Mesh", "Components", "VertexFaces", "MeshView", "weld", "MAX_TRIANGLES"]

MAX_TRIANGLES = 1 << 29
_INT32_MAX = int(np.iinfo(np.int32).max)
_ST_BOUND, _ST_BAD_INDEX, _ST_BAD_VERTEX = 7, 8, 16


def _raise_status(status, what):
    if status & _ST_BAD_VERTEX:
        raise ValueError(f"{what}: a vertex is not finite or its cell index leaves int32 (it joined no cluster, its faces were dropped)")
    if status & _ST_BAD_INDEX:
        raise ValueError(f"{what}: a face index lies outside 0 ... num_vertices - 1 (the face was skipped, nothing was indexed)")
    if status & _ST_BOUND:
        raise RuntimeError(f"{what}: a probe / find / retry loop reached its trip bound (status {status}); the result is not valid")


def _device_of(t):
    return t.device if t.device.index is not None else torch.device("cuda", torch.cuda.current_device())


def weld(vertices, colors=None, num_triangles=None, probe_stats=False):
    """-> Mesh. vertices: float32 [n,3,3] on the GPU, contiguous (a triangle soup); colors: None or the same shape;
    num_triangles: weld the first so many rows only (default: all). probe_stats: also sum the table slots every insertion
    looked at (Mesh.weld_probes; a diagnostic of tools/bench_mesh.py, it costs an atomic per wave)."""
    _call.check_tensor("vertices", vertices, "[n,3,3]", lambda t: t.dim() == 3 and tuple(t.shape[1:]) == (3, 3))
    _call.check_tensor("colors", colors, f"{tuple(vertices.shape)}", lambda t: t.shape == vertices.shape, none_ok=True)
    rows = int(vertices.shape[0])
    if num_triangles is None:
        num_triangles = rows
    if isinstance(num_triangles, bool) or not isinstance(num_triangles, (int, np.integer)) or not 0 <= num_triangles <= rows:
        raise ValueError(f"num_triangles must be an integer in 0 ... {rows}, got {num_triangles!r}")
    n = int(num_triangles)
    if n > MAX_TRIANGLES:
        raise ValueError(f"at most 2^29 triangles, got {n}")
    _call.check_gpu(vertices=vertices, colors=colors)
    dev = _device_of(vertices)
    _call.same_device(dev, "vertices' device", colors=colors)
    if not vertices.is_contiguous() or (colors is not None and not colors.is_contiguous()):
        raise ValueError("vertices and colors must be contiguous")
    lib = L.load()
    V = torch.empty((3 * n, 3), dtype=torch.float32, device=dev)
    Cc = None if colors is None else torch.empty((3 * n, 3), dtype=torch.float32, device=dev)
    F = torch.empty((n, 3), dtype=torch.int32, device=dev)
    state = torch.empty(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        scratch = _call.scratch(lib.sfgs_mesh_weld_scratch_bytes(n), dev, refused_if_zero=n > 0)
        L.check(lib.sfgs_mesh_weld(L.ptr(vertices.detach()), L.ptr(None if colors is None else colors.detach()), n, L.ptr(V), L.ptr(Cc),
                                   L.ptr(F), L.ptr(state), int(bool(probe_stats)), L.ptr(scratch), scratch.numel(), _call.stream(dev)))
    return Mesh._made(V, F, Cc, state, "weld")


class Components:
    """The result of Mesh.components, on the device. labels int32 [m]: the smallest vertex index of the vertex's component;
    triangles / vertices_in int32 [m]: per root (labels[r] == r) the faces whose first index lies in the component and its
    vertices, zero elsewhere; count: int64 [] the number of components."""

    def __init__(self, labels, triangles, vertices_in, state):
        self.labels, self.triangles, self.vertices_in, self._state = labels, triangles, vertices_in, state

    @property
    def count(self):
        return self._state[0]

    def check(self):
        """ONE host read: raises if the kernels left a status; -> the number of components as an int."""
        count, _, status, _ = self._state.tolist()
        _raise_status(status, "components")
        return count


class VertexFaces(tuple):
    """The result of Mesh.vertex_faces, on the device: the tuple (offsets int32 [m+1], records int32 [3n]). Vertex v's segment
    records[offsets[v]:offsets[v+1]] holds the corner records r = 3 t + c with faces[t][c] == v, ascending."""

    def __new__(cls, offsets, records, state):
        self = super().__new__(cls, (offsets, records))
        self.offsets, self.records, self._state = offsets, records, state
        return self

    def check(self):
        """ONE host read: raises if the kernels left a status (vertex_normals adds its own to it); -> the status, 0."""
        status = int(self._state[2])
        _raise_status(status, "vertex_faces")
        return status


class MeshView:
    """The result of Mesh.render, on the device. depth: float32 [1,H,W], 0 where no face covers the pixel; face: int32 [H,W], the
    index of the visible face, -1 where none; normal: float32 [3,H,W] in the world frame, zeros where depth is 0, or None; rgb:
    float32 [3,H,W], zeros where depth is 0, or None when the mesh has no colours; counts: int64 [4], the faces drawn, culled,
    clipped (a vertex unusable: not finite, at or in front of near, beyond the guard band) and degenerate (zero area after the
    snap). An ordinary view: depth goes into add_views, evaluate_dsm, sfgs.pointcloud, sfgs.ortho and ViewSet."""

    def __init__(self, depth, face, normal, rgb, state):
        self.depth, self.face, self.normal, self.rgb, self._state = depth, face, normal, rgb, state

    @property
    def counts(self):
        """int64 [4] on the device: drawn, culled, clipped, degenerate"""
        return self._state[:4]

    def check(self):
        """ONE host read: raises if the kernels left a status; -> (drawn, culled, clipped, degenerate) as ints."""
        words = self._state.tolist()
        _raise_status(words[4], "render")
        return tuple(words[:4])


class Mesh:
    """An indexed triangle mesh on the device. Mesh(vertices, faces, colors=None) takes a caller's mesh: vertices float32 [m,3],
    faces int32 [n,3], colors None or float32 [m,3], all contiguous on one GPU; the face indices are vetted on the device and a
    bad one is reported by the first use of a sized view, components() or clean().
    vertex_buffer / face_buffer / color_buffer: the storage, rows at or beyond the counts never written."""

    def __init__(self, vertices, faces, colors=None):
        _call.check_tensor("vertices", vertices, "[m,3]", lambda t: t.dim() == 2 and t.shape[1] == 3)
        _call.check_tensor("faces", faces, "[n,3]", lambda t: t.dim() == 2 and t.shape[1] == 3, dtypes=(torch.int32,))
        _call.check_tensor("colors", colors, f"{tuple(vertices.shape)}", lambda t: t.shape == vertices.shape, none_ok=True)
        m, n = int(vertices.shape[0]), int(faces.shape[0])
        if m > _INT32_MAX or n > MAX_TRIANGLES:
            raise ValueError(f"at most 2^31 - 1 vertices and 2^29 faces, got {m} and {n}")
        if n > 0 and m == 0:
            raise ValueError(f"{n} faces over no vertex")
        _call.check_gpu(vertices=vertices, faces=faces, colors=colors)
        dev = _device_of(vertices)
        _call.same_device(dev, "vertices' device", faces=faces, colors=colors)
        if not (vertices.is_contiguous() and faces.is_contiguous() and (colors is None or colors.is_contiguous())):
            raise ValueError("vertices, faces and colors must be contiguous")
        lib = L.load()
        state = torch.empty(4, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.sfgs_mesh_vet(L.ptr(faces), n, m, L.ptr(state), _call.stream(dev)))
        self._set(vertices.detach(), faces, None if colors is None else colors.detach(), state, "Mesh")

    def _set(self, V, F, Cc, state, what):
        self.vertex_buffer, self.face_buffer, self.color_buffer, self._state, self._what = V, F, Cc, state, what
        self._sizes_read = None
        self.device = V.device

    @classmethod
    def _made(cls, V, F, Cc, state, what):
        self = cls.__new__(cls)
        self._set(V, F, Cc, state, what)
        return self

    @property
    def num_vertices(self):
        """int64 [] on the device"""
        return self._state[0]

    @property
    def num_faces(self):
        """int64 [] on the device"""
        return self._state[1]

    def _sizes(self):
        if self._sizes_read is None:                      # ONE host read
            m, n, status, aux = self._state.tolist()
            _raise_status(status, self._what)
            assert 0 <= m <= self.vertex_buffer.shape[0] and 0 <= n <= self.face_buffer.shape[0], (m, n)
            self._sizes_read, self._aux = (m, n), aux
        return self._sizes_read

    @property
    def weld_probes(self):
        """The table slots the weld's insertions looked at in all (weld(..., probe_stats=True); for a decimated mesh the cluster
        insertions of decimate(..., probe_stats=True)), an int; 0 otherwise."""
        self._sizes()
        return self._aux

    @property
    def vertices(self):
        """float32 [m,3] on the device: a view of the valid rows"""
        return self.vertex_buffer[:self._sizes()[0]]

    @property
    def faces(self):
        """int32 [n,3] on the device"""
        return self.face_buffer[:self._sizes()[1]]

    @property
    def colors(self):
        """float32 [m,3] on the device, or None"""
        return None if self.color_buffer is None else self.color_buffer[:self._sizes()[0]]

    def components(self):
        """-> Components. Four launches, nothing read back beyond this mesh's own sizes."""
        m, n = self._sizes()
        dev, lib = self.device, L.load()
        labels, triangles, vertices_in = (torch.empty(m, dtype=torch.int32, device=dev) for _ in range(3))
        state = torch.empty(4, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            scratch = _call.scratch(lib.sfgs_mesh_components_scratch_bytes(m), dev, refused_if_zero=True)
            L.check(lib.sfgs_mesh_components(L.ptr(self.face_buffer), n, m, L.ptr(labels), L.ptr(triangles), L.ptr(vertices_in),
                                             L.ptr(state), L.ptr(scratch), scratch.numel(), _call.stream(dev)))
        return Components(labels, triangles, vertices_in, state)

    def clean(self, min_triangles=None, largest=None, drop_degenerate=False, components=None):
        """-> a new Mesh with the components below min_triangles faces and those beyond the first `largest` (by triangles
        descending, label ascending) removed, with drop_degenerate also the faces with two equal indices, and then every vertex
        that no kept face references. components: a components() result of THIS mesh, to save recomputing it; labels are not
        recomputed after faces were dropped. Outputs have this mesh's sizes; a clean that keeps everything equals its input."""
        for name, v in (("min_triangles", min_triangles), ("largest", largest)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0):
                raise ValueError(f"{name} must be None or a non-negative integer, got {v!r}")
        if not isinstance(drop_degenerate, (bool, np.bool_)):
            raise ValueError(f"drop_degenerate must be a bool, got {drop_degenerate!r}")
        if components is not None and not isinstance(components, Components):
            raise ValueError(f"components must be a components() result, got {components!r}")
        m, n = self._sizes()
        if components is not None and (components.labels.shape[0] != m or components.labels.device != self.device):
            raise ValueError("components were made for another mesh")
        dev, lib = self.device, L.load()
        cc = self.components() if components is None else components
        with torch.cuda.device(dev):
            # the component rule, on the device: plumbing over m integers, no host read
            is_root = cc.labels == torch.arange(m, dtype=torch.int32, device=dev)
            keep_root = is_root.clone()
            if min_triangles is not None:
                keep_root &= cc.triangles >= int(min(min_triangles, _INT32_MAX))
            if largest is not None:
                key = torch.where(is_root, -cc.triangles.to(torch.int64), torch.ones((), dtype=torch.int64, device=dev))
                order = torch.sort(key, stable=True).indices[:min(int(largest), m)]          # roots first, ties by ascending label
                top = torch.zeros(m, dtype=torch.bool, device=dev)
                top[order] = True
                keep_root &= top
            keep_root = keep_root.to(torch.uint8)
            V = torch.empty((m, 3), dtype=torch.float32, device=dev)
            Cc = None if self.color_buffer is None else torch.empty((m, 3), dtype=torch.float32, device=dev)
            F = torch.empty((n, 3), dtype=torch.int32, device=dev)
            state = torch.empty(4, dtype=torch.int64, device=dev)
            scratch = _call.scratch(lib.sfgs_mesh_clean_scratch_bytes(m, n), dev, refused_if_zero=True)
            L.check(lib.sfgs_mesh_clean(L.ptr(self.vertex_buffer), L.ptr(self.color_buffer), L.ptr(self.face_buffer), m, n,
                                        L.ptr(cc.labels), L.ptr(keep_root), int(bool(drop_degenerate)), L.ptr(V), L.ptr(Cc), L.ptr(F),
                                        L.ptr(state), L.ptr(scratch), scratch.numel(), _call.stream(dev)))
        return Mesh._made(V, F, Cc, state, "clean")

    def decimate(self, cell, origin=(0.0, 0.0, 0.0), drop_duplicates=True, return_map=False, probe_stats=False):
        """-> a new Mesh (with return_map: (Mesh, int32 [m] on the device: the output index of each input vertex's cluster, -1
        when it was dropped or the vertex was bad)) by vertex clustering on the grid of `cell` at `origin`; the module's docstring
        and include/sfgs.h state the result. Outputs have this mesh's sizes; nothing is read back beyond this mesh's own sizes.
        probe_stats: also sum the table slots the cluster insertions looked at (the result's weld_probes; a diagnostic)."""
        if isinstance(cell, bool) or not isinstance(cell, (int, float, np.integer, np.floating)) or not np.isfinite(cell) or cell <= 0:
            raise ValueError(f"cell must be a finite number > 0, got {cell!r}")
        org = _vec(origin, 3, "origin")
        if not np.isfinite(org).all():
            raise ValueError(f"origin must be finite, got {origin!r}")
        for name, v in (("drop_duplicates", drop_duplicates), ("return_map", return_map), ("probe_stats", probe_stats)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"{name} must be a bool, got {v!r}")
        m, n = self._sizes()
        dev, lib = self.device, L.load()
        with torch.cuda.device(dev):
            V = torch.empty((m, 3), dtype=torch.float32, device=dev)
            Cc = None if self.color_buffer is None else torch.empty((m, 3), dtype=torch.float32, device=dev)
            F = torch.empty((n, 3), dtype=torch.int32, device=dev)
            vmap = torch.empty(m, dtype=torch.int32, device=dev) if return_map else None
            state = torch.empty(4, dtype=torch.int64, device=dev)
            scratch = _call.scratch(lib.sfgs_mesh_decimate_scratch_bytes(m, n, int(Cc is not None)), dev, refused_if_zero=True)
            L.check(lib.sfgs_mesh_decimate(L.ptr(self.vertex_buffer), L.ptr(self.color_buffer), L.ptr(self.face_buffer), m, n, float(cell),
                                           float(org[0]), float(org[1]), float(org[2]), int(bool(drop_duplicates)) | 2 * int(bool(probe_stats)),
                                           L.ptr(V), L.ptr(Cc), L.ptr(F), L.ptr(vmap), L.ptr(state), L.ptr(scratch), scratch.numel(),
                                           _call.stream(dev)))
        out = Mesh._made(V, F, Cc, state, "decimate")
        return (out, vmap) if return_map else out

    def vertex_faces(self):
        """-> VertexFaces, the tuple (offsets int32 [m+1], records int32 [3n]) on the device: the vertex -> face inverted index
        over the corner records r = 3 t + c, every segment ascending (np.argsort(F.reshape(-1), kind="stable") and the
        cumulative counts). A face that names a vertex twice appears twice in its segment."""
        m, n = self._sizes()
        dev, lib = self.device, L.load()
        with torch.cuda.device(dev):
            offsets = torch.empty(m + 1, dtype=torch.int32, device=dev)
            records = torch.empty(3 * n, dtype=torch.int32, device=dev)
            state = torch.empty(4, dtype=torch.int64, device=dev)
            scratch = _call.scratch(lib.sfgs_mesh_vertex_faces_scratch_bytes(m), dev, refused_if_zero=True)
            L.check(lib.sfgs_mesh_vertex_faces(L.ptr(self.face_buffer), n, m, L.ptr(offsets), L.ptr(records), L.ptr(state), L.ptr(scratch),
                                               scratch.numel(), _call.stream(dev)))
        return VertexFaces(offsets, records, state)

    def vertex_normals(self, adjacency=None):
        """-> float32 [m,3] on the device: per vertex the float64 sum of its faces' area-weighted normals (b - a) x (c - a), taken
        in ascending order of the corner records and normalised; (0, 0, 0) where the sum has no finite positive length.
        adjacency: a vertex_faces() result of THIS mesh, to save rebuilding it."""
        if adjacency is not None and not isinstance(adjacency, VertexFaces):
            raise ValueError(f"adjacency must be a vertex_faces() result, got {adjacency!r}")
        m, n = self._sizes()
        if adjacency is not None and (adjacency.offsets.shape[0] != m + 1 or adjacency.records.shape[0] != 3 * n or
                                      adjacency.offsets.device != self.device):
            raise ValueError("adjacency was made for another mesh")
        adj = self.vertex_faces() if adjacency is None else adjacency
        dev, lib = self.device, L.load()
        with torch.cuda.device(dev):
            normals = torch.empty((m, 3), dtype=torch.float32, device=dev)
            L.check(lib.sfgs_mesh_vertex_normals(L.ptr(self.vertex_buffer), L.ptr(self.face_buffer), m, n, L.ptr(adj.offsets),
                                                 L.ptr(adj.records), L.ptr(normals), L.ptr(adj._state), _call.stream(dev)))
        return normals

    def render(self, camera, height, width, near=0.0, far=math.inf, normals=True, cull=None, out=None, _small_max=None):
        """-> MeshView: the mesh seen from `camera` at height x width pixels -- depth along the forward axis (0 where no face
        covers the pixel), the index of the visible face (-1), its normal in the world frame and, when the mesh has colours, the
        interpolated colour -- with four launches and nothing read back beyond this mesh's own sizes. camera: read as
        TsdfVolume.raycast reads one (R, T, focal_x, focal_y; cx, cy default to 0). near, far: a face with a vertex at or in
        front of `near` is not drawn (there is no near-plane clipping), a pixel deeper than `far` is not kept. normals: True =
        the visible face's flat normal (winding as stored), a float32 [m,3] tensor on the mesh's device (vertex_normals()) = the
        interpolated vertex normals, False = none. cull: None draws both sides, "back" only the faces whose normal points
        toward the camera. out: a MeshView of an earlier call with the same arguments, written again in place.
        _small_max: private; the box size in pixels up to which a face is rasterised by its own thread (every value gives the
        same bytes)."""
        for name, v in (("height", height), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        H, W = int(height), int(width)
        if H * W > 1 << 30:
            raise ValueError(f"height * width must not exceed 2^30, got {H} x {W}")
        near = _positive(near, "near", at_least=0.0)
        far = _positive(far, "far", allow_inf=True)
        if not far > near:
            raise ValueError(f"far must be above near, got near {near}, far {far}")
        if cull not in (None, "back"):
            raise ValueError(f"cull must be None or 'back', got {cull!r}")
        if _small_max is not None and (isinstance(_small_max, bool) or not isinstance(_small_max, (int, np.integer)) or
                                       not 0 <= _small_max <= 1 << 30):
            raise ValueError(f"_small_max must be None or an integer in 0 ... 2^30, got {_small_max!r}")
        rows = int(self.vertex_buffer.shape[0])
        vnormals = None
        if isinstance(normals, torch.Tensor):
            vnormals = normals
            _call.check_tensor("normals", vnormals, "[m,3]", lambda t: t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous())
            _call.check_gpu(normals=vnormals)
            _call.same_device(self.device, "the mesh's device", normals=vnormals)
        elif not isinstance(normals, (bool, np.bool_)):
            raise ValueError(f"normals must be a bool or a float32 [m,3] tensor, got {normals!r}")
        want_normal, colours = vnormals is not None or bool(normals), self.color_buffer is not None
        if out is not None:
            if not isinstance(out, MeshView):
                raise ValueError(f"out must be a MeshView, got {out!r}")
            if (out.normal is not None) != want_normal or (out.rgb is not None) != colours:
                raise ValueError("out was made with other normals or by a mesh with other colours")
            _call.check_tensor("out.depth", out.depth, f"[1,{H},{W}]", lambda t: tuple(t.shape) == (1, H, W) and t.is_contiguous())
            _call.check_tensor("out.face", out.face, f"[{H},{W}]", lambda t: tuple(t.shape) == (H, W) and t.is_contiguous(),
                               dtypes=(torch.int32,))
            for name, t in (("out.normal", out.normal), ("out.rgb", out.rgb)):
                _call.check_tensor(name, t, f"[3,{H},{W}]", lambda t: tuple(t.shape) == (3, H, W) and t.is_contiguous(), none_ok=True)
            _call.check_tensor("out state", out._state, "[8]", lambda t: tuple(t.shape) == (8,), dtypes=(torch.int64,))
        try:
            cam = (camera.R, camera.T, camera.focal_x, camera.focal_y, getattr(camera, "cx", 0.0), getattr(camera, "cy", 0.0))
        except AttributeError as e:
            raise ValueError(f"camera: {e}") from None
        dev = self.device
        view = out
        if view is None:
            view = MeshView(torch.empty((1, H, W), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.int32, device=dev),
                            torch.empty((3, H, W), dtype=torch.float32, device=dev) if want_normal else None,
                            torch.empty((3, H, W), dtype=torch.float32, device=dev) if colours else None,
                            torch.empty(8, dtype=torch.int64, device=dev))
        # the view's checks on the depth map that will be written: its size, its device, the camera's numbers
        _, _, (M, c, _, cx_pix, cy_pix, fx, fy) = _check_view(dev, view.depth, *cam, None, None, centre_from_view=True, face=view.face,
                                                              normal=view.normal, rgb=view.rgb, state=view._state)
        m, n = self._sizes()
        if vnormals is not None and int(vnormals.shape[0]) not in (m, rows):
            raise ValueError(f"normals must have a row per vertex ({m}), got {int(vnormals.shape[0])}")
        lib = L.load()
        args = L.SfgsMeshRender(L.C.sizeof(L.SfgsMeshRender), H, W, 0 if cull is None else 1, M, c, cx_pix, cy_pix, fx, fy, near, far,
                                m, n, -1 if _small_max is None else int(_small_max), self.vertex_buffer.data_ptr(),
                                None if not colours else self.color_buffer.data_ptr(), self.face_buffer.data_ptr(),
                                None if vnormals is None else vnormals.data_ptr(), view.depth.data_ptr(), view.face.data_ptr(),
                                None if view.normal is None else view.normal.data_ptr(),
                                None if view.rgb is None else view.rgb.data_ptr(), view._state.data_ptr())
        with torch.cuda.device(dev):
            scratch = _call.scratch(lib.sfgs_mesh_render_scratch_bytes(m, n, H, W), dev, refused_if_zero=True)
            L.check(lib.sfgs_mesh_render(L.C.byref(args), L.ptr(scratch), scratch.numel(), _call.stream(dev)))
        return view

    def save_ply(self, path, origin=None, normals=None):
        """Binary little-endian PLY in TriangleSoup.save_ply's layout: a `vertex` and a `face` element (`property list uchar int
        vertex_indices`), vertices `double` with origin (added in float64) and `float` without, with colours `uchar red / green /
        blue` by (x * 255 + 0.5).clip(0, 255), NaN -> 0. normals: float32 [m,3] on the mesh's device (vertex_normals()); they
        go in as `float nx / ny / nz` after z and before the colours."""
        org = None if origin is None else _vec(origin, 3, "origin")
        V = np.ascontiguousarray(self.vertices.cpu().numpy())
        if normals is not None:
            if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or tuple(normals.shape) != (len(V), 3):
                raise ValueError(f"normals must be a float32 tensor of shape ({len(V)}, 3)")
            if normals.device != self.vertex_buffer.device:
                raise ValueError(f"normals must be on the mesh's device {self.vertex_buffer.device}, got {normals.device}")
        F = np.ascontiguousarray(self.faces.cpu().numpy())
        if len(V) > _INT32_MAX:
            raise ValueError(f"{len(V)} vertices do not fit the PLY's int indices")
        kind, ftype = ("double", "<f8") if org is not None else ("float", "<f4")
        fields = [(a, ftype) for a in "xyz"]
        header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(V)}"] + [f"property {kind} {a}" for a in "xyz"]
        if normals is not None:
            fields += [(a, "<f4") for a in ("nx", "ny", "nz")]
            header += [f"property float {a}" for a in ("nx", "ny", "nz")]
        if self.color_buffer is not None:
            fields += [(c, "u1") for c in ("red", "green", "blue")]
            header += [f"property uchar {c}" for c in ("red", "green", "blue")]
        header += [f"element face {len(F)}", "property list uchar int vertex_indices", "end_header"]
        vt = np.empty(len(V), dtype=fields)
        for j, a in enumerate("xyz"):
            vt[a] = V[:, j] if org is None else V[:, j].astype(np.float64) + org[j]
        if normals is not None:
            nv = normals.detach().cpu().numpy()
            for j, a in enumerate(("nx", "ny", "nz")):
                vt[a] = nv[:, j]
        if self.color_buffer is not None:
            c = np.ascontiguousarray(self.colors.cpu().numpy())
            with np.errstate(invalid="ignore"):
                q = np.where(np.isnan(c), np.float32(0), (c * np.float32(255) + np.float32(0.5)).clip(0, 255)).astype(np.uint8)
            for j, name in enumerate(("red", "green", "blue")):
                vt[name] = q[:, j]
        ft = np.empty(len(F), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        ft["n"], ft["i"] = 3, F
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(path, "wb") as f:
            f.write(("\n".join(header) + "\n").encode("ascii"))
            vt.tofile(f)
            ft.tofile(f)
