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

Queries (csrc/mesh_query.hip; include/sfgs.h in words, tests/mesh_query_np.py in numpy; byte for byte as well):

    grid = clean.face_grid(cell=2 * voxel, origin=vol_origin, dims=(nx // 2, ny // 2, nz // 2))   # FaceGrid: a CSR table of faces per cell
    d = clean.closest(points, grid, max_distance=4 * voxel)                  # MeshDistance: sqdist float64 [k], face int32 [k]
    answered, without, left_out = d.check()                                  # ONE host read
    pts = small.sample(density=1 / voxel ** 2, seed=0)                       # MeshSamples: points, face, colors, uniform per area
    error = clean.closest(pts.points).distance                               # how far the decimated surface lies from the full one

The cell of a coordinate is floor((x - origin) / cell) in float64, for faces and queries alike. A face is registered in every
cell its box overlaps (clamped into the grid); one whose range holds more than 4096 cells goes to a large list that every query
tests; one with an index out of range or a vertex that is not finite is left out and counted. closest answers, per point, the
minimum over all faces not left out of (squared distance to the closed triangle in float64, face index): it tests the large
list, then the Chebyshev rings of cells around the point's own cell from the first that meets the grid, and stops after ring r
once best < (r cell)^2 (1 - 2^-20) -- a face in no visited cell is at least r cell away, because the cell function is monotone
and shared -- or r cell (1 - 2^-20) > max_distance. The grid changes no byte of the answer. One thread per query: a wave per
query was measured (profiles/r27_mesh_distance_ab.txt: a quarter faster against the 4 M-face mesh, 3 - 5.5 x slower elsewhere)
and is kept as tools/variants/mesh_query_wave.patch; bucketing the queries by cell was not built. Without a grid the cell is default_cell()'s: max(sqrt(S / n),
L / 512), S half the surface of the bounds, L their longest side. sample gives face t floor(e) + (u < e - floor(e)) points, e =
area x density, u and the positions from a 32-bit integer mixer of (seed, face, counter): the same bytes for the same seed.
d.summary(thresholds) reduces a result in one launch and one host read: exact counts per threshold, mean, RMS and max from
float64 sums formed in a fixed order (the same bytes run after run); compare(a, b, density, max_distance, thresholds) samples
both meshes, queries each one's samples against the other and gives the Chamfer distance, precision, recall and F-score. Timings: tools/bench_mesh_distance.py, profiles/r27_mesh_distance_ab.txt.

There is no hole filling or smoothing, and no torch fallback: without the HIP library every operator raises."""
import math
import os

import numpy as np
import torch

from . import _call
from . import _lib as L
from .geometry import _check_view, _vec
from .tsdf import _positive

__all__ = ["Mesh", "Components", "VertexFaces", "MeshView", "FaceGrid", "MeshDistance", "MeshSamples", "DistanceSummary",
           "MeshComparison", "weld", "compare", "grid_from_bounds", "default_cell", "MAX_TRIANGLES", "MAX_GRID_CELLS"]

MAX_TRIANGLES = 1 << 29
MAX_GRID_CELLS = 1 << 28
MAX_THRESHOLDS = 16
_INT32_MAX = int(np.iinfo(np.int32).max)
_ST_BOUND, _ST_BAD_INDEX, _ST_BAD_VERTEX = 7, 8, 16
_ST_CAPACITY, _ST_PAIRS, _ST_BAD_FACE = 32, 64, 128


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


def _raise_query_status(status, what, need=None, capacity=None):
    if status & _ST_PAIRS:
        raise ValueError(f"{what}: more than 2^31 - 1 entries ({need}); use a larger cell or a smaller density")
    if status & _ST_CAPACITY:
        raise ValueError(f"{what}: {need} (face, cell) pairs found, capacity {capacity}: the pairs beyond it were dropped and the "
                         f"table is not valid; a capacity of {need} would have sufficed")
    if status & _ST_BAD_FACE:
        raise ValueError(f"{what}: a face has an area that is not finite, or more than 2^20 samples (it sampled nothing)")
    _raise_status(status, what)


def grid_from_bounds(box, cell):
    """-> (origin float64 [3], dims): the face grid over the bounds `box` = (lo, hi): origin = lo, dims = floor((hi - lo) / cell)
    + 1 per axis in float64; a mesh without a usable face (box None) gets one cell at the origin."""
    if box is None:
        return np.zeros(3), (1, 1, 1)
    lo, hi = (np.asarray(b, dtype=np.float64) + 0.0 for b in box)           # + 0.0: a minimum of -0.0 and +0.0 is +0.0 either way
    dims = tuple(int(d) for d in np.floor((hi - lo) / np.float64(cell)) + 1.0)
    return lo, dims


def default_cell(box, n):
    """The cell Mesh.closest picks without a grid: max(sqrt(S / n), L / 512) with (ex, ey, ez) = the extent of the bounds, S =
    ex ey + ey ez + ez ex (half the box's surface: a surface of n faces inside it then has about a face per cell it passes
    through) and L the longest extent (at most 512^3 = 2^27 cells); 1 when that is not positive."""
    if box is None or n < 1:
        return 1.0
    ex, ey, ez = (float(h) - float(l) for l, h in zip(*box))
    cell = max(math.sqrt((ex * ey + ey * ez + ez * ex) / n), max(ex, ey, ez) / 512.0)
    return cell if cell > 0.0 and math.isfinite(cell) else 1.0


class FaceGrid:
    """The result of Mesh.face_grid, on the device: a uniform grid over the faces as a CSR table. cell, origin (float64 [3]),
    dims (nx, ny, nz); cell (x, y, z) has the index (z ny + y) nx + x. cell_start: int32 [nx ny nz + 1]; pairs: int32
    [capacity], the faces of cell c at cell_start[c]:cell_start[c + 1], ascending; large: int32 [n], the faces whose cell range
    was larger than max_cells, in no particular order (num_large of them), which every query tests."""

    def __init__(self, mesh, cell, origin, dims, cell_start, pairs, large, state, args):
        self.mesh, self.cell, self.origin, self.dims = mesh, cell, origin, dims
        self.cell_start, self.pairs, self.large, self._state, self._args = cell_start, pairs, large, state, args

    @property
    def num_pairs(self):
        """int64 [] on the device: the (face, cell) pairs in all -- the capacity needed"""
        return self._state[0]

    @property
    def num_large(self):
        """int64 [] on the device"""
        return self._state[1]

    @property
    def skipped(self):
        """int64 [] on the device: the faces left out (an index out of range, a coordinate that is not finite)"""
        return self._state[3]

    def check(self):
        """ONE host read: raises if the capacity was too small (naming the number needed) or the kernels left another status;
        -> (pairs, large, skipped) as ints."""
        pairs, large, status, skipped = self._state.tolist()
        _raise_query_status(status, "face_grid", pairs, int(self.pairs.shape[0]))
        return pairs, large, skipped


class MeshDistance:
    """The result of Mesh.closest, on the device. sqdist: float64 [k], the squared distance to the closest face, +inf where
    there is none; face: int32 [k], its index, -1 where none (no face at all, one beyond max_distance, a point that is not
    finite); point: float32 [k,3], the closest point, or None; grid: the FaceGrid that was searched."""

    def __init__(self, sqdist, face, point, state, grid):
        self.sqdist, self.face, self.point, self._state, self.grid = sqdist, face, point, state, grid

    @property
    def counts(self):
        """int64 [3] on the device: the queries answered, those without a face, the faces the grid left out"""
        return self._state[[0, 1, 3]]

    @property
    def distance(self):
        """float64 [k]: sqrt(sqdist)"""
        return torch.sqrt(self.sqdist)

    def check(self):
        """ONE host read: raises if the kernel left a status; -> (answered, without a face, faces left out) as ints."""
        answered, without, status, skipped = self._state.tolist()
        _raise_query_status(status, "closest")
        return answered, without, skipped

    def summary(self, thresholds=()):
        """-> DistanceSummary over the ANSWERED queries, d = sqrt(sqdist): one reduction launch and ONE host read. thresholds: up
        to 16 numbers >= 0; per threshold the exact count of answered queries with d <= it. The sums of d and d^2 are float64,
        formed in a fixed order (include/sfgs.h): the same bytes run after run."""
        try:
            taus = [float(t) for t in thresholds]
        except (TypeError, ValueError):
            raise ValueError(f"thresholds must be a sequence of numbers, got {thresholds!r}") from None
        if len(taus) > MAX_THRESHOLDS or not all(t >= 0 for t in taus):
            raise ValueError(f"thresholds must be at most {MAX_THRESHOLDS} numbers >= 0, got {thresholds!r}")
        k, dev, lib = int(self.sqdist.shape[0]), self.sqdist.device, L.load()
        with torch.cuda.device(dev):
            out = torch.empty(4 + MAX_THRESHOLDS, dtype=torch.int64, device=dev)
            scratch = _call.scratch(lib.sfgs_mesh_distance_summary_scratch_bytes(k), dev, refused_if_zero=True)
            L.check(lib.sfgs_mesh_distance_summary(L.ptr(self.sqdist), L.ptr(self.face), k, (L.C.c_double * max(len(taus), 1))(*taus),
                                                   len(taus), L.ptr(out), L.ptr(scratch), scratch.numel(), _call.stream(dev)))
        words = np.array(out.tolist(), dtype=np.int64)              # ONE host read
        sums = words[:3].view(np.float64)
        return DistanceSummary(k, int(words[3]), float(sums[0]), float(sums[1]), float(sums[2]), tuple(taus),
                               tuple(int(c) for c in words[4:4 + len(taus)]))


class DistanceSummary:
    """The result of MeshDistance.summary, on the host. queries; answered; sum_d, sum_d2, max: float64 over the answered queries;
    thresholds and counts (answered queries with d <= threshold, exact). mean and rms are over the answered queries (NaN without
    one); fractions are counts / QUERIES: a query without an answer is farther than every threshold."""

    def __init__(self, queries, answered, sum_d, sum_d2, max_d, thresholds, counts):
        self.queries, self.answered, self.sum_d, self.sum_d2, self.max = queries, answered, sum_d, sum_d2, max_d
        self.thresholds, self.counts = thresholds, counts
        self.mean = sum_d / answered if answered else math.nan
        self.rms = math.sqrt(sum_d2 / answered) if answered else math.nan
        self.fractions = tuple(c / queries if queries else math.nan for c in counts)


class MeshComparison:
    """The result of compare(a, b, ...): a_to_b / b_to_a: the DistanceSummary of a's samples against b and of b's against a;
    chamfer: the mean of the two means; per threshold precision (a's samples within it of b), recall (b's within it of a) and
    fscore = 2 P R / (P + R), 0 where both are 0."""

    def __init__(self, a_to_b, b_to_a):
        self.a_to_b, self.b_to_a = a_to_b, b_to_a
        self.chamfer = 0.5 * (a_to_b.mean + b_to_a.mean)
        self.precision, self.recall = a_to_b.fractions, b_to_a.fractions
        self.fscore = tuple(2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(self.precision, self.recall))


def compare(a, b, density, max_distance=None, thresholds=(), seed=0):
    """-> MeshComparison of two meshes on one device: both are sampled at `density` (Mesh.sample with `seed`), each one's samples
    are queried against the other (Mesh.closest with `max_distance`) and summarised (MeshDistance.summary with `thresholds`).
    Plain Python over those three; it costs their host reads."""
    if not isinstance(a, Mesh) or not isinstance(b, Mesh):
        raise ValueError("compare takes two Mesh objects")
    if a.device != b.device:
        raise ValueError(f"the meshes must be on one device, got {a.device} and {b.device}")
    pa, pb = a.sample(density, seed=seed, colors=False).points, b.sample(density, seed=seed, colors=False).points
    return MeshComparison(b.closest(pa, max_distance=max_distance).summary(thresholds),
                          a.closest(pb, max_distance=max_distance).summary(thresholds))


class MeshSamples:
    """The result of Mesh.sample, on the device. point_buffer float32 [capacity,3], face_buffer int32 [capacity], color_buffer
    float32 [capacity,3] or None: rows at or beyond `count` never written; points / face / colors: the sized views (ONE host
    read on first use, which raises when the capacity was too small or a face could not be sampled)."""

    def __init__(self, points, face, colors, state, capacity):
        self.point_buffer, self.face_buffer, self.color_buffer, self._state, self.capacity = points, face, colors, state, capacity
        self._count_read = None

    @property
    def count(self):
        """int64 [] on the device: the samples FOUND (more than `capacity` when the buffers were too small)"""
        return self._state[0]

    def _count(self):
        if self._count_read is None:                      # ONE host read
            k, _, status, _ = self._state.tolist()
            _raise_query_status(status, "sample", k)
            if k > self.capacity:
                raise ValueError(f"MeshSamples: {k} samples found, capacity {self.capacity}: the rows beyond it were dropped; "
                                 f"a capacity of {k} would have sufficed")
            self._count_read = k
        return self._count_read

    @property
    def points(self):
        return self.point_buffer[:self._count()]

    @property
    def face(self):
        return self.face_buffer[:self._count()]

    @property
    def colors(self):
        return None if self.color_buffer is None else self.color_buffer[:self._count()]


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

    # ---- queries: the face grid, the closest face, points on the surface (csrc/mesh_query.hip) -------------------------------
    def _grid_bounds(self, m, n):
        """-> (lo [3], hi [3]) float64: the bounds of the vertices that the faces not left out reference; None when there are
        none. A device reduction over plumbing tensors and ONE host read."""
        if n == 0:
            return None
        V, F = self.vertex_buffer[:m], self.face_buffer[:n]
        big = torch.full((3,), math.inf, dtype=torch.float32, device=self.device)
        lo, hi = big.clone(), -big
        for i in range(0, n, 1 << 20):                              # a million faces at a time: tens of megabytes, not hundreds
            Fc = F[i:i + (1 << 20)].to(torch.int64)
            ok = ((Fc >= 0) & (Fc < m)).all(dim=1)
            P = V[Fc.clamp(0, m - 1)]                               # [c,3,3]
            ok &= torch.isfinite(P).all(dim=2).all(dim=1)
            lo = torch.minimum(lo, torch.where(ok[:, None, None], P, big).amin(dim=(0, 1)))
            hi = torch.maximum(hi, torch.where(ok[:, None, None], P, -big).amax(dim=(0, 1)))
        words = torch.cat([lo, hi]).to(torch.float64).tolist()      # ONE host read
        if not all(math.isfinite(w) for w in words):
            return None
        return np.array(words[:3]), np.array(words[3:])

    def face_grid(self, cell, origin=None, dims=None, capacity=None, _max_cells=None, _bounds=False):
        """-> FaceGrid: a uniform grid of `cell` over the faces as a CSR table (the module's docstring and include/sfgs.h state
        it). origin, dims: the grid's corner and its cell counts (nx, ny, nz), as a TSDF volume's; None for both: the bounds of
        the referenced finite vertices, origin = their minimum and dims = floor((max - origin) / cell) + 1 per axis, by a device
        reduction and one host read. capacity: the length of `pairs`; None sizes it by ONE host read of the pair total between
        count and fill; an integer costs no read, and one too small is reported by FaceGrid.check().
        _max_cells: private; a face whose range holds more cells goes to the large list (every value gives the same answers)."""
        cell = _positive(cell, "cell")
        if (origin is None) != (dims is None):
            raise ValueError("origin and dims come together")
        if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or
                                     not 0 <= capacity <= _INT32_MAX):
            raise ValueError(f"capacity must be None or an integer in 0 ... 2^31 - 1, got {capacity!r}")
        if _max_cells is not None and (isinstance(_max_cells, bool) or not isinstance(_max_cells, (int, np.integer)) or
                                       not 0 <= _max_cells <= 1 << 30):
            raise ValueError(f"_max_cells must be None or an integer in 0 ... 2^30, got {_max_cells!r}")
        m, n = self._sizes()
        if origin is None:
            box = self._grid_bounds(m, n) if _bounds is False else _bounds       # _bounds: closest() has read them already
            org, dims = grid_from_bounds(box, cell)
        else:
            org = _vec(origin, 3, "origin")
            if not np.isfinite(org).all():
                raise ValueError(f"origin must be finite, got {origin!r}")
            try:
                dims = tuple(int(d) for d in dims)
            except (TypeError, ValueError):
                raise ValueError(f"dims must be three integers, got {dims!r}") from None
        if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > MAX_GRID_CELLS:
            raise ValueError(f"dims must be three integers >= 1 with at most 2^28 cells in all, got {dims!r}")
        cells = dims[0] * dims[1] * dims[2]
        dev, lib = self.device, L.load()
        with torch.cuda.device(dev):
            cell_start = torch.empty(cells + 1, dtype=torch.int32, device=dev)
            large = torch.empty(n, dtype=torch.int32, device=dev)
            state = torch.empty(4, dtype=torch.int64, device=dev)
            args = L.SfgsMeshGrid(L.C.sizeof(L.SfgsMeshGrid), dims[0], dims[1], dims[2], (L.C.c_double * 3)(*[float(x) for x in org]),
                                  cell, m, n, -1 if _max_cells is None else int(_max_cells), 0, self.vertex_buffer.data_ptr(),
                                  self.face_buffer.data_ptr(), cell_start.data_ptr(), None, large.data_ptr(), state.data_ptr())
            scratch = _call.scratch(lib.sfgs_mesh_grid_scratch_bytes(*dims), dev, refused_if_zero=True)
            L.check(lib.sfgs_mesh_grid_count(L.C.byref(args), L.ptr(scratch), scratch.numel(), _call.stream(dev)))
            if capacity is None:
                total, _, status, _ = state.tolist()                # ONE host read
                if status & _ST_PAIRS:
                    raise ValueError(f"face_grid: {total} (face, cell) pairs, more than 2^31 - 1: use a larger cell")
                capacity = total
            pairs = torch.empty(int(capacity), dtype=torch.int32, device=dev)
            args.capacity, args.pairs = int(capacity), pairs.data_ptr()
            L.check(lib.sfgs_mesh_grid_fill(L.C.byref(args), L.ptr(scratch), scratch.numel(), _call.stream(dev)))
        return FaceGrid(self, cell, org, dims, cell_start, pairs, large, state, args)

    def closest(self, points, grid=None, max_distance=None, closest_points=False, _max_cells=None):
        """-> MeshDistance: for each point the closest face of the mesh and the squared distance to it, in float64 (the module's
        docstring and include/sfgs.h state the answer; it does not depend on the grid). points: float32 or float64 [k,3] on the
        mesh's device, contiguous. grid: a face_grid() result of THIS mesh, a cell size (a grid is built over the mesh's
        bounds), or None: a grid with the cell default_cell() picks from the bounds and the face count. max_distance: an
        answer farther away is reported as face -1 and sqdist +inf. closest_points: also the closest point, float32 [k,3]."""
        _call.check_tensor("points", points, "[k,3]", lambda t: t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous(),
                           dtypes=(torch.float32, torch.float64))
        _call.check_gpu(points=points)
        _call.same_device(self.device, "the mesh's device", points=points)
        if max_distance is None:
            max_distance = math.inf
        if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float, np.integer, np.floating)) or not max_distance >= 0:
            raise ValueError(f"max_distance must be None or a number >= 0, got {max_distance!r}")
        if isinstance(grid, FaceGrid):
            if grid.mesh is not self:
                raise ValueError("grid was made for another mesh")
            if _max_cells is not None:
                raise ValueError("_max_cells goes with a grid built here")
        elif grid is None:
            m, n = self._sizes()
            box = self._grid_bounds(m, n)
            grid = self.face_grid(default_cell(box, n), _max_cells=_max_cells, _bounds=box)
        else:
            grid = self.face_grid(grid, _max_cells=_max_cells)
        k = int(points.shape[0])
        dev, lib = self.device, L.load()
        with torch.cuda.device(dev):
            sqdist = torch.empty(k, dtype=torch.float64, device=dev)
            face = torch.empty(k, dtype=torch.int32, device=dev)
            point = torch.empty((k, 3), dtype=torch.float32, device=dev) if closest_points else None
            state = torch.empty(4, dtype=torch.int64, device=dev)
            L.check(lib.sfgs_mesh_closest(L.C.byref(grid._args), L.ptr(points.detach()), int(points.dtype == torch.float64), k,
                                          float(max_distance), L.ptr(sqdist), L.ptr(face), L.ptr(point), L.ptr(state), _call.stream(dev)))
        return MeshDistance(sqdist, face, point, state, grid)

    def sample(self, density, seed=0, capacity=None, colors=True):
        """-> MeshSamples: points on the surface, uniform per area, `density` per unit of area on average, the same bytes for the
        same seed (the module's docstring and include/sfgs.h state them), ordered by face. capacity: the rows of the outputs; a
        row beyond it is not written but still counted, as TsdfVolume.extract does; None counts first and costs ONE host read.
        colors: also the interpolated colours when the mesh has them."""
        if isinstance(density, bool) or not isinstance(density, (int, float, np.integer, np.floating)) or not np.isfinite(density) or \
                density < 0:
            raise ValueError(f"density must be a finite number >= 0, got {density!r}")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 1 << 32:
            raise ValueError(f"seed must be an integer in 0 ... 2^32 - 1, got {seed!r}")
        if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or
                                     not 1 <= capacity <= _INT32_MAX):
            raise ValueError(f"capacity must be None or an integer in 1 ... 2^31 - 1, got {capacity!r}")
        m, n = self._sizes()
        dev, lib = self.device, L.load()
        with_colors = bool(colors) and self.color_buffer is not None
        with torch.cuda.device(dev):
            state = torch.empty(4, dtype=torch.int64, device=dev)
            scratch = _call.scratch(lib.sfgs_mesh_sample_scratch_bytes(n), dev, refused_if_zero=True)

            def run(cap, points, face, cols):
                L.check(lib.sfgs_mesh_sample(L.ptr(self.vertex_buffer), L.ptr(self.color_buffer), L.ptr(self.face_buffer), m, n,
                                             float(density), int(seed), cap, L.ptr(points), L.ptr(face), L.ptr(cols), L.ptr(state),
                                             L.ptr(scratch), scratch.numel(), _call.stream(dev)))
            if capacity is None:
                run(0, None, None, None)                            # counts only
                capacity, _, status, _ = state.tolist()             # ONE host read
                _raise_query_status(status, "sample")
            capacity = int(capacity)
            points = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
            face = torch.empty(capacity, dtype=torch.int32, device=dev)
            cols = torch.empty((capacity, 3), dtype=torch.float32, device=dev) if with_colors else None
            if capacity > 0:
                run(capacity, points, face, cols)
        return MeshSamples(points, face, cols, state, capacity)

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
