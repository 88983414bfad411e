"""Shared by test_scene_edit_host.py and test_gpu_scene_edit.py: the arithmetic of
vr_scene_transform_mesh restated in numpy from the formulas of include/vanrijn_amd.h, and matrices.

numpy's elementwise products and sums are separate IEEE operations (no contraction), evaluated in the
order written here, which is the header's.
"""
import copy
import math

import numpy as np

IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def cofactor(matrix):
    """K[i][j] = A[i+1][j+1] * A[i+2][j+2] - A[i+1][j+2] * A[i+2][j+1], indices mod 3, in Python floats."""
    m = [float(x) for x in np.asarray(matrix, dtype=np.float64).reshape(-1)]
    a = [[m[4 * i + j] for j in range(3)] for i in range(3)]
    return [[a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3] -
             a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3] for j in range(3)] for i in range(3)]


def transformed(matrix, vertices, normals):
    """T_M of [n][3][3] vertices and normals: what vr_scene_transform_mesh stores, bit for bit."""
    m = [float(x) for x in np.asarray(matrix, dtype=np.float64).reshape(-1)]
    assert len(m) == 12
    k = cofactor(m)
    v = np.asarray(vertices, dtype=np.float64)
    n = np.asarray(normals, dtype=np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    with np.errstate(over="ignore", invalid="ignore"):
        out_v = np.stack([((m[4 * c] * x + m[4 * c + 1] * y) + m[4 * c + 2] * z) + m[4 * c + 3] for c in range(3)],
                         axis=-1)
        out_n = np.stack([(k[c][0] * nx + k[c][1] * ny) + k[c][2] * nz for c in range(3)], axis=-1)
    return np.ascontiguousarray(out_v), np.ascontiguousarray(out_n)


def rotation_y(angle, translation=(0.0, 0.0, 0.0)):
    """A rotation about the vertical axis plus a translation, row-major 3x4."""
    c, s = math.cos(angle), math.sin(angle)
    return [c, 0.0, s, translation[0], 0.0, 1.0, 0.0, translation[1], -s, 0.0, c, translation[2]]


def rotation_about(angle, centre, shift=(0.0, 0.0, 0.0)):
    """Rotate about the vertical axis through `centre`, then shift."""
    c, s = math.cos(angle), math.sin(angle)
    cx, cy, cz = centre
    return [c, 0.0, s, cx - (c * cx + s * cz) + shift[0], 0.0, 1.0, 0.0, shift[1],
            -s, 0.0, c, cz - (-s * cx + c * cz) + shift[2]]


MATRICES = {
    "rotation": [0.36, 0.48, -0.8, 0.25, -0.8, 0.6, 0.0, -1.5, 0.48, 0.64, 0.6, 2.0],  # orthonormal rows, det +1
    "scale": [2.5, 0.0, 0.0, 0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0, 1.7, 0.0],
    "reflection": [-1.0, 0.0, 0.0, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0],
    "zero": [0.0] * 12,
}
OVERFLOW = [1e308, 0.0, 0.0, 0.0, 0.0, 1e308, 0.0, 0.0, 0.0, 0.0, 1e308, 0.0]
SINGULAR = [1.0, 0.5, 0.0, -1.0, 2.0, 1.0, 0.0, 0.0, -1.0, -0.5, 0.0, 0.5]  # rank 1: every triangle on one line


def edited_spec(spec, camera=None, primitives=None, materials=None, meshes=None, integrator=None):
    """A copy of `spec` with the given replacements: primitives {(object, position): PrimitiveSpec},
    materials {index: MaterialSpec}, meshes {index: (vertices, normals)}."""
    from vanrijn_amd.scene import MeshSpec, ObjectSpec
    out = copy.copy(spec)
    if camera is not None:
        out.camera_location = tuple(float(c) for c in camera)
    out.materials = list(spec.materials)
    for i, m in (materials or {}).items():
        out.materials[i] = m
    out.objects = [ObjectSpec(o.kind, list(o.primitives), o.mesh) for o in spec.objects]
    for (oi, k), p in (primitives or {}).items():
        out.objects[oi].primitives[k] = p
    out.meshes = list(spec.meshes)
    for i, (v, n) in (meshes or {}).items():
        out.meshes[i] = MeshSpec(np.ascontiguousarray(v), np.ascontiguousarray(n), spec.meshes[i].material)
    if integrator is not None:
        out.integrator = integrator
    return out


def rows_equal(a, b):
    """Structured arrays equal byte for byte."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
