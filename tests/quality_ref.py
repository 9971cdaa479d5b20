"""The tree-quality measure of a CWBVH (PTMeasureGeometry / PTMeasureBVHArrays, include/ptmi_plugin.h Part 10)
restated in numpy float64, for the tests.

Written from the rule, not from the C++:

  reachable   the nodes reached from node 0 through the inner slots (meta & 0x1F >= 24), each node's inner children consecutive
              from childBase in slot order; levels = the depth of that walk
  slot        occupied iff its meta byte is not 0; extent per axis (q_hi - q_lo) * 2^e, e the axis' signed exponent byte;
              halfArea = ex*ey + ey*ez + ez*ex; weight 1 for an inner slot, popcount(meta >> 5) for a leaf slot
  root        the fold of the root's occupied slots' decoded boxes lo + q * 2^e; rootHalfArea is the half area of that box
  cost        1 + sum over every occupied slot of every reachable node of halfArea / rootHalfArea * weight; 0 when rootHalfArea is 0
"""
import numpy as np

import lbvh_ref


def half_area(e):
    return e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]


def measure(nodes, triangle_count):
    """nodes: flat uint8 (80 bytes per node; unreachable nodes may follow).  Returns the dict PTMeasureBVHArrays fills."""
    n = np.asarray(nodes, np.uint8).reshape(-1, 80)
    levels = lbvh_ref.levels_of(n)
    reach = np.concatenate(levels)
    r = n[reach]
    cell = np.exp2(r[:, 12:15].copy().view(np.int8).astype(np.float64))                # (nodes, 3)
    meta = r[:, 24:32]
    q_lo = r[:, 32:56].reshape(-1, 3, 8).astype(np.float64)                            # [node, axis, slot]
    q_hi = r[:, 56:80].reshape(-1, 3, 8).astype(np.float64)
    ext = np.moveaxis((q_hi - q_lo) * cell[:, :, None], 1, 2)                          # [node, slot, axis]
    unary = (meta >> 5).astype(np.int64)
    weight = np.where((meta & 0x1F) >= 24, 1, (unary & 1) + ((unary >> 1) & 1) + ((unary >> 2) & 1))
    weight = np.where(meta == 0, 0, weight).astype(np.float64)
    # the root's box
    used = meta[0] != 0
    origin = r[0, 0:12].copy().view(np.float32).astype(np.float64)
    if used.any():
        lo = (origin[:, None] + q_lo[0][:, used] * cell[0][:, None]).min(axis=1)
        hi = (origin[:, None] + q_hi[0][:, used] * cell[0][:, None]).max(axis=1)
        root = float(half_area(hi - lo))
    else:
        root = 0.0
    cost = 1.0 + float((half_area(ext) / root * weight).sum()) if root > 0 else 0.0
    return {"nodeCapacity": n.shape[0], "nodeCount": int(reach.size), "triangleCount": int(triangle_count), "levels": len(levels),
            "rootHalfArea": root, "sahCost": cost}
