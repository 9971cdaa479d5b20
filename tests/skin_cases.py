"""Procedural skins for the skinning tests (test_skin.py, test_gpu_skin.py): weights, joints, palettes and rest attributes."""
import numpy as np

from unity_webgpu_pathtracer_amd import abi


def rotation(rng):
    """A random rotation matrix (3, 3) float64"""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def palette(joint_count, seed, amplitude=1.0):
    """(J, 12) float32: a random rotation, a uniform scale in 0.5 ... 1.5 and a translation per joint.  amplitude < 1 keeps the pose
    near the identity (rotation angle, scale and translation all shrink with it)."""
    rng = np.random.RandomState(seed)
    out = np.zeros((joint_count, 3, 4))
    for j in range(joint_count):
        r = rotation(rng)
        r = np.eye(3) + amplitude * (r - np.eye(3)) if amplitude < 1.0 else r
        out[j, :, :3] = r * (1.0 + amplitude * rng.uniform(-0.5, 0.5))
        out[j, :, 3] = amplitude * rng.uniform(-1, 1, 3)
    return out.reshape(joint_count, 12).astype(np.float32)


def skin_of(vertices, joint_count, seed):
    """Joints (n, 4) uint16 and weights (n, 4) float32 for the vertices: random joints, weights that sum to about 1, a quarter of
    them exact zeros, and every eighth vertex one-hot."""
    rng = np.random.RandomState(seed)
    n = len(vertices)
    joints = rng.randint(0, joint_count, (n, 4)).astype(np.uint16)
    w = rng.uniform(0.05, 1.0, (n, 4))
    w[rng.uniform(size=(n, 4)) < 0.25] = 0.0
    w[:, 0] = np.where(w.sum(axis=1) == 0, 1.0, w[:, 0])
    w /= w.sum(axis=1, keepdims=True)
    w[::8] = 0.0
    w[::8, 1] = 1.0
    return joints, w.astype(np.float32)


def rest_attrs(triangle_count, seed, material_count=1):
    """T abi.TRI_ATTR records: unit normals and tangents, random uvs and pads, materialIndex below material_count"""
    rng = np.random.RandomState(seed)
    a = np.zeros(triangle_count, abi.TRI_ATTR)
    rows = a.view(np.float32).reshape(-1, 8, 4)
    rows[:] = rng.uniform(-1, 1, rows.shape)
    d = rows[:, :6, :3]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    a["materialIndex"] = rng.randint(0, material_count, triangle_count)
    return a
