"""PathTracer's scene and geometry updates (include/ptmi_plugin.h Parts 5 and 9 to 12): instances, lights, materials, vertices,
skins and morph targets, refitted or rebuilt in place."""
import ctypes as C
import warnings
from dataclasses import replace

import numpy as np

from . import abi, plugin
from ._hostcalls import HostCalls, torch
from .scenes import instance_world_bounds


class Updates(HostCalls):
    # ---- scene updates (include/ptmi_plugin.h Part 5)
    def set_instance_transforms(self, local_to_world) -> bool:
        """Move the instances (one 4x4 localToWorld each): BVHScene.UpdateTLAS, then Reset() when anything changed, as the
        reference's frame loop does (PathTracer.cs:169-183).  Returns whether anything changed."""
        changed = self._bvhScene.UpdateTLAS(self.ctx, local_to_world)
        if changed:
            self.Reset()
        return changed

    def update_instances_device(self, records):
        """PTUpdateInstancesDevice from a torch tensor on this context's device holding instanceCount PTBlasInstance records
        (192 bytes each, e.g. uint8 (n, 192) or float32 (n, 48)).  Ordered after torch's current stream; torch's later work
        is ordered after the update.  Does not reset accumulation."""
        assert records.is_contiguous() and records.numel() * records.element_size() % 192 == 0
        n = records.numel() * records.element_size() // 192
        with self._ordered(records.device):
            plugin.check(self.lib.PTUpdateInstancesDevice(self.ctx, records.data_ptr(), n))

    def update_lights(self, lights: np.ndarray):
        """PTUpdateLights: (k, 16) float32 PTLight records, 1 <= k <= the scene's light count."""
        L = np.ascontiguousarray(lights, dtype=np.float32).reshape(-1, 16)
        plugin.check(self.lib.PTUpdateLights(self.ctx, L.ctypes.data, L.shape[0]))
        self._lightRecords = L.copy()           # what light_records() and muted_lights() (Part 24) start from

    def update_materials(self, materials: np.ndarray):
        """PTUpdateMaterials: (materialCount, 32) float32 PTMaterialData records."""
        M = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, 32)
        plugin.check(self.lib.PTUpdateMaterials(self.ctx, M.ctypes.data, M.shape[0]))

    def read_tlas(self):
        """PTReadTLAS: the current TLAS as plugin.build_tlas returns it -> (node bytes uint8[], indices uint32[])."""
        n = self._bvhScene.gpu_instances.shape[0]
        nodes = np.empty((2 * n - 1) * 64, np.uint8)
        idx = np.empty(n, np.uint32)
        count = C.c_uint32()
        plugin.check(self.lib.PTReadTLAS(self.ctx, nodes.ctypes.data, nodes.nbytes, idx.ctypes.data, n, C.byref(count)))
        return nodes[:count.value * 64].copy(), idx

    # ---- geometry updates (include/ptmi_plugin.h Part 9)
    def _built_cost(self, mesh):
        """sahCost after the BLAS's last build or rebuild; the tree as built is measured on the host from the arrays PTSetScene was given"""
        if mesh not in self._builtCost:
            bvh = self._bvhScene
            n0, cap, t0, nt = bvh.blas_spans[0 if mesh is None else mesh]
            self._builtCost[mesh] = plugin.measure_cwbvh((bvh.bvh_nodes[n0 * 80:(n0 + cap) * 80], bvh.bvh_tris[t0 * 16:t0 * 16 + nt * 48]), nt)["sahCost"]
        return self._builtCost[mesh]

    def _refit_or_rebuild(self, mesh, refit, rebuild, rebuild_above=None, force=False):
        """The policy the three geometry calls share.  refit() runs, and with rebuild_above (a ratio) PTMeasureGeometry follows:
        if sahCost exceeds rebuild_above x the cost recorded after the BLAS's last build or rebuild, rebuild() runs on the same
        input.  force: rebuild() alone.  Every rebuild records the new tree's cost in _builtCost.  Returns (what the call that ran
        last returned, "refit" or "rebuild")."""
        if not force:
            res = refit()
            if rebuild_above is None or self.geometry_quality(mesh)["sahCost"] <= rebuild_above * self._built_cost(mesh):
                return res, "refit"
        res = rebuild()
        self._builtCost[mesh] = self.geometry_quality(mesh)["sahCost"]
        return res, "rebuild"

    def rebuild_geometry(self, vertices, mesh: int = None, tri_attrs=None):
        """PTRebuildGeometry / PTRebuildGeometryDevice: update_geometry's contract, but the BLAS gets a new tree (the device
        builder's, built in place on the GPU) instead of a refit.  The tree must fit the BLAS's node span (node_capacity)."""
        self._refit_or_rebuild(mesh, None, lambda: self._set_vertices(vertices, mesh, tri_attrs, True), force=True)

    def geometry_quality(self, mesh: int = None) -> dict:
        """PTMeasureGeometry: nodeCapacity, nodeCount, triangleCount, levels, rootHalfArea and sahCost of the BLAS's current tree.
        Synchronising."""
        q = abi.geometry_quality()
        plugin.check(self.lib.PTMeasureGeometry(self.ctx, *self._blas_offsets(mesh), C.byref(q)))
        return q.as_dict()

    def update_geometry(self, vertices, mesh: int = None, tri_attrs=None, rebuild_above: float = None):
        """PTUpdateGeometry: new positions for one BLAS, refitted in place on the GPU.  vertices: (3 * triangles, 4) float32 in
        the BLAS's primitive order (numpy), or a torch tensor on this context's device (PTUpdateGeometryDevice, ordered after
        torch's current stream; tri_attrs then is a device tensor too).  tri_attrs (optional): the BLAS's abi.TRI_ATTR records.
        Flat scene: mesh stays None.  HAS_TLAS scene: mesh indexes scene.mesh_ranges; the vertices are in the mesh's local space,
        and the world bounds of the mesh's instances are recomputed (scenes.instance_world_bounds) and sent through
        PTUpdateInstances -- the library does not touch the TLAS (with device tensors that is left to the caller).  Does not
        reset accumulation.
        rebuild_above (a ratio, no default): the refit is followed by PTMeasureGeometry; if sahCost exceeds rebuild_above x the cost
        recorded after the BLAS's last build or rebuild, the same vertices go through PTRebuildGeometry.  Returns "refit" or
        "rebuild" then, None otherwise."""
        _, what = self._refit_or_rebuild(mesh, lambda: self._set_vertices(vertices, mesh, tri_attrs, False),
                                         lambda: self._set_vertices(vertices, mesh, None, True),         # the attributes were replaced by the refit
                                         rebuild_above)
        return None if rebuild_above is None else what

    def _set_vertices(self, vertices, mesh, tri_attrs, rebuild):
        """update_geometry's call: PTUpdateGeometry, or with rebuild PTRebuildGeometry, and what follows it on the host"""
        bvh = self._bvhScene
        off = self._blas_offsets(mesh)
        fn_host, fn_device = (self.lib.PTRebuildGeometry, self.lib.PTRebuildGeometryDevice) if rebuild else (self.lib.PTUpdateGeometry, self.lib.PTUpdateGeometryDevice)
        if not isinstance(vertices, np.ndarray):
            assert vertices.is_contiguous() and vertices.dtype == torch.float32 and vertices.numel() % 12 == 0
            assert tri_attrs is None or (tri_attrs.is_contiguous() and tri_attrs.numel() * tri_attrs.element_size() == vertices.numel() // 12 * 128)
            with self._ordered(vertices.device):
                plugin.check(fn_device(self.ctx, *off, vertices.data_ptr(), vertices.numel() // 12, None if tri_attrs is None else tri_attrs.data_ptr()))
            if bvh.gpu_instances is not None:
                warnings.warn("update_geometry with device tensors on a HAS_TLAS scene: resend the instances' world bounds "
                              "(PTUpdateInstances / update_instances_device), the vertices are not read back for them")
            return
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        assert v.ndim == 2 and v.shape[1] == 4 and v.shape[0] % 3 == 0
        a = None if tri_attrs is None else np.ascontiguousarray(tri_attrs)
        assert a is None or a.nbytes == v.shape[0] // 3 * 128
        plugin.check(fn_host(self.ctx, *off, v.ctypes.data, v.shape[0] // 3, None if a is None else a.ctypes.data))
        # later transform updates take the mesh's bounds from the scene's vertices: kept current in a copy of our own, made once
        if not getattr(self, "_ownVertices", False):
            self.scene = bvh.scene = replace(self.scene, vertices=self.scene.vertices.copy())
            self._ownVertices = True
        t0 = 0 if mesh is None else self.scene.mesh_ranges[mesh][0]
        self.scene.vertices[t0 * 3:t0 * 3 + v.shape[0]] = v
        self._send_instance_bounds(mesh, v)

    def _send_instance_bounds(self, mesh, local):
        """HAS_TLAS: the world bounds of the mesh's instances from its local box -- `local` is the two corners (2, 3), or the
        vertices themselves (scenes.instance_world_bounds takes the extremes of either) --, through PTUpdateInstances"""
        bvh = self._bvhScene
        if bvh.gpu_instances is None:
            return
        for k, (m_, _, _) in enumerate(self.scene.instances):
            if m_ != mesh:
                continue
            l2w = bvh.gpu_instances[k]["localToWorld"].reshape(4, 4).T.astype(np.float64)
            bvh.blas_instances[k]["aabbMin"], bvh.blas_instances[k]["aabbMax"] = instance_world_bounds(local, l2w)
        plugin.check(self.lib.PTUpdateInstances(self.ctx, bvh.blas_instances.ctypes.data, bvh.blas_instances.shape[0]))

    def _deformed(self, mesh, rebuild, rebuild_above, call):
        """skin_geometry's and morph_geometry's tail: call(flags, out) fills the six floats of the deformed vertices' bounds -- as
        a refit, or under the rebuild policy --, which then move the mesh's instances.  Returns what the two return."""
        def run(flags):
            out = (C.c_float * 6)()
            call(flags, out)
            bounds = np.array(out, np.float32).reshape(2, 3)
            self._send_instance_bounds(mesh, bounds)
            return bounds
        bounds, what = self._refit_or_rebuild(mesh, lambda: run(0), lambda: run(abi.PT_SKIN_REBUILD), rebuild_above, force=rebuild and rebuild_above is None)
        return bounds if rebuild_above is None else (bounds, what)

    # ---- skinned geometry (include/ptmi_plugin.h Part 11)
    def set_skin(self, rest_vertices, joints, weights, mesh: int = None, rest_attrs=None, joint_count: int = None):
        """PTSetSkin: the skin of one BLAS, uploaded once.  rest_vertices (3T, 4) float32 in the BLAS's primitive order
        (update_geometry's layout), joints (3T, 4) uint16, weights (3T, 4) float32, rest_attrs (optional) the BLAS's abi.TRI_ATTR
        records of the rest pose -- with them every skin_geometry also writes the skinned normals and tangents.  joint_count: the
        palette's length (default: the largest joint index + 1).  rest_vertices = None removes the BLAS's skin."""
        off = self._blas_offsets(mesh)
        nt = self._bvhScene.blas_spans[0 if mesh is None else mesh][3]
        if rest_vertices is None:
            plugin.check(self.lib.PTSetSkin(self.ctx, *off, nt, None))
            return
        if joint_count is None:
            joint_count = int(np.asarray(joints).max()) + 1
        d, ntri, keep = plugin.skin_desc(rest_vertices, joints, weights, joint_count, rest_attrs)
        plugin.check(self.lib.PTSetSkin(self.ctx, *off, ntri, C.byref(d)))

    def skin_geometry(self, joint_matrices, mesh: int = None, rebuild: bool = False, rebuild_above: float = None):
        """PTSkinGeometry: one joint palette in, the BLAS's vertices skinned on the GPU and refitted (rebuild=True: rebuilt, Part
        10's rules) in place -- no vertex is uploaded or read back.  joint_matrices: numpy (J, 3, 4) or (J, 12) (rest space to the
        mesh's local space: joint world x inverse bind), or a float32 torch tensor of that shape on this context's device
        (PTSkinGeometryDevice, ordered after torch's current stream).  Returns the skinned vertices' bounds, (2, 3) float32: min, max.
        HAS_TLAS scene: the world bounds of the mesh's instances are recomputed from those two corners
        (scenes.instance_world_bounds) and sent through PTUpdateInstances.  Does not reset accumulation.
        rebuild_above: update_geometry's policy -- refit, measure, and rebuild from the same palette if sahCost exceeds
        rebuild_above x the cost after the BLAS's last build or rebuild; returns (bounds, "refit" or "rebuild") then."""
        off = self._blas_offsets(mesh)

        def call(flags, out):
            if isinstance(joint_matrices, np.ndarray):
                m = plugin.joint_palette(joint_matrices)
                plugin.check(self.lib.PTSkinGeometry(self.ctx, *off, m.ctypes.data, m.shape[0], flags, out))
            else:
                m = joint_matrices
                assert m.is_contiguous() and m.dtype == torch.float32 and m.numel() % 12 == 0 and tuple(m.shape[1:]) in ((3, 4), (12,))
                with self._ordered(m.device):
                    plugin.check(self.lib.PTSkinGeometryDevice(self.ctx, *off, m.data_ptr(), m.numel() // 12, flags, out))
        return self._deformed(mesh, rebuild, rebuild_above, call)

    # ---- morph targets (include/ptmi_plugin.h Part 12)
    def set_morph(self, rest_vertices, position_deltas, normal_deltas=None, tangent_deltas=None, mesh: int = None, rest_attrs=None,
                  target_count: int = None):
        """PTSetMorph: the morph targets of one BLAS, uploaded once.  rest_vertices (3T, 4) float32 in the BLAS's primitive order
        (update_geometry's layout).  Each deltas argument is a dense (K, 3T, 3) float32 array (converted by plugin.morph_csr: a corner
        lists a target unless its delta is exactly +0, +0, +0) or an (offsets, entries) CSR tuple; normal_deltas and tangent_deltas
        need rest_attrs, the BLAS's abi.TRI_ATTR records of the rest pose -- with rest_attrs every morph_geometry also writes the
        records.  target_count: default the dense array's K, or for a CSR position stream its largest target + 1.
        rest_vertices = None removes the BLAS's morph."""
        off = self._blas_offsets(mesh)
        nt = self._bvhScene.blas_spans[0 if mesh is None else mesh][3]
        if rest_vertices is None:
            plugin.check(self.lib.PTSetMorph(self.ctx, *off, nt, None))
            return
        if target_count is None:
            if isinstance(position_deltas, tuple):
                target_count = int(np.asarray(position_deltas[1])["target"].max()) + 1 if len(position_deltas[1]) else 1
            else:
                target_count = len(position_deltas)
        d, ntri, keep = plugin.morph_desc(rest_vertices, target_count, position_deltas, normal_deltas, tangent_deltas, rest_attrs)
        plugin.check(self.lib.PTSetMorph(self.ctx, *off, ntri, C.byref(d)))

    def morph_geometry(self, weights, joint_matrices=None, mesh: int = None, rebuild: bool = False, rebuild_above: float = None):
        """PTMorphGeometry: one weight per target in (and optionally skin_geometry's joint palette: morph first, then the skin), the
        BLAS's vertices made on the GPU and refitted (rebuild=True: rebuilt, Part 10's rules) in place -- no vertex is uploaded or
        read back.  weights: numpy (K,), joint_matrices numpy (J, 3, 4) or (J, 12) or None; or float32 torch tensors on this
        context's device (PTMorphGeometryDevice, ordered after torch's current stream; both on the device then).  Returns the
        vertices' bounds, (2, 3) float32: min, max.  HAS_TLAS scene: the world bounds of the mesh's instances are recomputed from
        those two corners and sent through PTUpdateInstances.  Does not reset accumulation.
        rebuild_above: update_geometry's policy; returns (bounds, "refit" or "rebuild") then."""
        off = self._blas_offsets(mesh)

        def call(flags, out):
            if isinstance(weights, np.ndarray):
                w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
                m = None if joint_matrices is None else plugin.joint_palette(joint_matrices)
                plugin.check(self.lib.PTMorphGeometry(self.ctx, *off, w.ctypes.data, len(w), None if m is None else m.ctypes.data,
                                                      0 if m is None else m.shape[0], flags, out))
            else:
                w, m = weights, joint_matrices
                assert w.is_contiguous() and w.dtype == torch.float32 and w.dim() == 1
                assert m is None or (m.is_contiguous() and m.dtype == torch.float32 and m.numel() % 12 == 0 and tuple(m.shape[1:]) in ((3, 4), (12,)))
                with self._ordered(w.device):
                    plugin.check(self.lib.PTMorphGeometryDevice(self.ctx, *off, w.data_ptr(), w.numel(), None if m is None else m.data_ptr(),
                                                                0 if m is None else m.numel() // 12, flags, out))
        return self._deformed(mesh, rebuild, rebuild_above, call)

    def read_geometry(self):
        """PTReadGeometry: the current (nodes uint8[], tris uint8[], tri_attrs abi.TRI_ATTR[]) of the whole scene.  Synchronising."""
        bvh = self._bvhScene
        nodes, tris = np.empty(bvh.bvh_nodes.nbytes, np.uint8), np.empty(bvh.bvh_tris.nbytes, np.uint8)
        attrs = np.empty(bvh.tri_attrs.shape, bvh.tri_attrs.dtype)
        plugin.check(self.lib.PTReadGeometry(self.ctx, nodes.ctypes.data, nodes.nbytes, tris.ctypes.data, tris.nbytes, attrs.ctypes.data, attrs.nbytes))
        return nodes, tris, attrs
