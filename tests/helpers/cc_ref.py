"""Host reference of the mesh component stage (text2nerf_amd.mesh.mesh_components / filter_components) over
`scipy.sparse.csgraph.connected_components`: the canonical renumbering (dense labels in the order of each component's smallest vertex
index), the counts, the keep rule (min_faces, keep_largest with ties to the lower label) and an order-preserving filter. Plus the test
volumes of tests/test_mesh_components_*.py. Nothing here runs on the device."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

f32 = np.float32


def components(faces, n_verts):
    """(labels [V] int32, K, vert_counts [K] int32, face_counts [K] int32). Two vertices are connected when a face contains both; a
    vertex that no face references is a component of its own with 0 faces; a face counts for the component of its vertices."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = int(n_verts)
    if V == 0:
        e = np.zeros(0, np.int32)
        return e, 0, e.copy(), e.copy()
    a = np.concatenate([f[:, 0], f[:, 1]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    graph = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(V, V))
    K, raw = connected_components(graph, directed=False)
    # scipy's numbering is its own: renumber by the smallest vertex of each component = the first place its raw label occurs
    _, first = np.unique(raw, return_index=True)
    rank = np.empty(K, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(K)
    labels = rank[raw].astype(np.int32)
    vert_counts = np.bincount(labels, minlength=K).astype(np.int32)
    face_counts = np.bincount(labels[f[:, 0]], minlength=K).astype(np.int32)
    return labels, int(K), vert_counts, face_counts


def keep_mask(face_counts, min_faces=0, keep_largest=None):
    """Component c stays iff face_counts[c] >= min_faces and, with keep_largest = k, c is among the k components with the most faces;
    ties go to the lower label."""
    fc = np.asarray(face_counts, dtype=np.int64)
    keep = fc >= min_faces
    if keep_largest is not None:
        order = np.argsort(-fc, kind="stable")
        top = np.zeros(len(fc), bool)
        top[order[:keep_largest]] = True
        keep &= top
    return keep


def filter_mesh(verts, faces, normals, colors, labels, keep):
    """The vertices of kept components in their order (rows of verts / normals / colors together), the faces of kept components in
    their order, re-indexed."""
    labels = np.asarray(labels)
    keep = np.asarray(keep, dtype=bool)
    kv = keep[labels] if len(labels) else np.zeros(0, bool)
    newidx = np.cumsum(kv) - 1
    f = np.asarray(faces).reshape(-1, 3)
    kf = kv[f[:, 0]] if len(f) else np.zeros(0, bool)
    rows = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x)[kv])
    return rows(verts), newidx[f[kf]].astype(np.int32).reshape(-1, 3), rows(normals), rows(colors)


# ---- test volumes -----------------------------------------------------------------------------------------------------------------
def _grid(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")


def _segment_distance(p, a, b):
    """Distance of the points p [...,3] from the segment a-b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = b - a
    t = np.clip(((p - a) @ d) / float(d @ d), 0.0, 1.0)
    return np.linalg.norm(p - (a + t[..., None] * d), axis=-1)


def serpentine_volume(shape, rows, z, radius=1.2, x0=4.0, x1=None):
    """radius - distance from one polyline: along axis 0 from x0 to x1 on each of `rows` (y), the rows joined at alternating ends, at
    height z. Level 0 is a tube, one component, whose vertex order (node-linear: axis 0 slowest) crosses every row again and again."""
    x1 = shape[0] - 5.0 if x1 is None else x1
    pts = []
    for k, y in enumerate(rows):
        ends = [(x0, y, z), (x1, y, z)]
        pts += ends if k % 2 == 0 else ends[::-1]
    p = np.stack(_grid(shape), -1)
    dist = np.full(shape, np.inf)
    for a, b in zip(pts[:-1], pts[1:]):
        dist = np.minimum(dist, _segment_distance(p, a, b))
    return (radius - dist).astype(f32)


BLOBS = (((10.3, 10.1, 11.2), (7.0, 6.0, 8.5)), ((29.6, 9.7, 12.4), (4.0, 5.0, 4.5)), ((28.2, 18.3, 4.6), (1.6, 1.4, 1.7)))
BLOB_SHAPE, BLOB_SPACING, BLOB_ORIGIN = (40, 22, 24), (0.3, 0.7, 1.1), (-2.0, 1.0, 0.5)


def blob_volume(which):
    """The ellipsoid(s) BLOBS[i] for i in `which` in a 40 x 22 x 24 box, each clipped below at -0.25 (so that far from a blob the
    volume is flat and the blobs do not shape each other's neighbourhood), combined by max."""
    from tests.helpers import mc_ref
    vols = [np.maximum(mc_ref.ellipsoid_volume(BLOB_SHAPE, c=BLOBS[i][0], r=BLOBS[i][1]), f32(-0.25)) for i in which]
    return np.maximum.reduce(vols).astype(f32)
