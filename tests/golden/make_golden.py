#!/usr/bin/env python3
"""Generates the committed golden fixtures (run in the build container, where /root/reference exists).

  cwbvh_*.npz   byte-exact CWBVH node/triangle dumps and TLAS dumps produced by the REFERENCE plugin
                (Assets/Plugins/Web/plugin.cpp compiled in place -> oracle/_ref), together with their inputs.
  trace_*.npz   rays + (t, prim) from the REFERENCE's tinybvh CPU walker BVH::Intersect (oracle/ref_driver.cpp).
  trace_cwbvh_*.npz  rays + (t, u, v, prim) from the REFERENCE's own CWBVH walker BVH8_CWBVH::Intersect
                (oracle/ref_driver_cwbvh.cpp) -- the CPU twin of the shader's RayIntersectBvh.
  frame_*.npz   frames rendered by the CPU oracle (regression pin of the restatement itself; the reference's
                shader cannot be executed here, so these are NOT reference outputs -- see DESIGN.md).
  ref_builds.npz, ref_walker_sponza03.npz, ref_cwbvh_walker_sponza03.npz  what the reference plugin and its two walkers
                return for the inputs of the *_live tests (tests/test_bvh_builder.py, tests/test_oracle.py), which use them
                where oracle/_ref is not built: `--only live`.
  helmet_geometry.npz  the reference snapshot's one real model, Assets/Examples/Models/DamagedHelmet.glb, as a .glb
                with its images emptied (JSON chunk + geometry buffer views only): `--only helmet PATH_TO_GLB`.

Fixtures are data only (inputs and expected outputs); no reference source text is stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402
from unity_webgpu_pathtracer_amd import abi, scenes  # noqa: E402


def soup(rng, n, spread=10.0, size=1.0):
    c = rng.uniform(-spread, spread, (n, 1, 3))
    v = c + rng.normal(0, size, (n, 3, 3))
    out = np.zeros((n * 3, 4), np.float32)
    out[:, :3] = v.reshape(-1, 3)
    return out


def gen_trace_cwbvh():
    """trace_cwbvh_*.npz: rays + full hit records (t, u, v, prim) from the reference's OWN CWBVH walker,
    BVH8_CWBVH::Intersect (tiny_bvh.h:7006-7114) through oracle/ref_driver_cwbvh.cpp, with the CRC-32 of the node and
    triangle bytes that walker traversed (= the bytes BuildBVH must produce for the same scene)."""
    import zlib
    rng = np.random.RandomState(20261005)
    for name, sc, box, nr in (("zoo", scenes.material_zoo(), ((-3.5, 0.2, -3.5), (3.5, 4.0, 3.5)), 4000),
                              ("sponza03", scenes.sponza_atrium(tex_size=4, detail=0.3), ((-14, 0.3, -6.5), (14, 11, 6.5)), 6000)):
        rays = np.zeros((nr, 8), np.float32)
        rays[:, 0:3] = rng.uniform(box[0], box[1], (nr, 3))
        d = rng.normal(0, 1, (nr, 3))
        rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
        rays[:, 6] = 1e5
        rec, rn, rt = pyoracle.ref_cwbvh_trace(sc.vertices, rays)
        np.savez_compressed(os.path.join(HERE, f"trace_cwbvh_{name}.npz"), rays=rays, records=rec,
                            node_crc=np.uint32(zlib.crc32(rn.tobytes())), tri_crc=np.uint32(zlib.crc32(rt.tobytes())))
        print(f"trace_cwbvh_{name}: {nr} rays, hits {int((rec[:, 3].view(np.uint32) != 0xFFFFFFFF).sum())}")


def main():
    pyoracle.build(ref=True)
    rng = np.random.RandomState(20251226)
    cases = {
        "cornell": scenes.cornell_box().vertices,
        "soup1": soup(rng, 1), "soup3": soup(rng, 3), "soup4": soup(rng, 4), "soup300": soup(rng, 300, 6.0, 0.5),
        "flat_grid": scenes.SoupBuilder(),
    }
    sb = cases.pop("flat_grid")
    sb.quad((-2, 0, -2), (4, 0, 0), (0, 0, 4), (0, 1, 0), 6, 6, 0)
    cases["flat_grid72"] = sb.finish()[0]
    dup = np.zeros((60, 4), np.float32)
    dup[:, :3] = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (20, 1))
    cases["identical20"] = dup
    for name, v in cases.items():
        nodes, tris = pyoracle.ref_build_cwbvh(v)
        np.savez_compressed(os.path.join(HERE, f"cwbvh_{name}.npz"), vertices=v, nodes=nodes, tris=tris)
        print(f"cwbvh_{name}: {v.shape[0] // 3} tris -> {nodes.nbytes} node bytes, {tris.nbytes} tri bytes")
    for n in (1, 2, 5, 40):
        inst = np.zeros(n, abi.BLAS_INSTANCE)
        c = rng.uniform(-20, 20, (n, 3))
        e = rng.uniform(0.1, 3, (n, 3))
        inst["aabbMin"] = c - e
        inst["aabbMax"] = c + e
        nodes, idx = pyoracle.ref_build_tlas(inst)
        np.savez_compressed(os.path.join(HERE, f"tlas_{n}.npz"), instances=inst.view(np.uint8), nodes=nodes, indices=idx)
        print(f"tlas_{n}: {nodes.nbytes} node bytes")

    # reference CPU traversal known-answers on a small scene
    s = scenes.material_zoo()
    ref = pyoracle.load_ref_tinybvh()
    import ctypes as C
    verts = np.ascontiguousarray(s.vertices, np.float32)
    h = ref.ref_bvh_build(verts.ctypes.data_as(C.c_void_p), s.tri_count, None)
    n = 4000
    o = rng.uniform(-3.5, 3.5, (n, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(0.2, 4.0, n)
    d = rng.normal(0, 1, (n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, 1e5
    rays[n // 2:, 7] = 1.0
    t = np.zeros(n, np.float32)
    prim = np.zeros(n, np.uint32)
    ref.ref_bvh_trace(h, rays.ctypes.data_as(C.c_void_p), n, 1, t.ctypes.data_as(C.c_void_p), prim.ctypes.data_as(C.c_void_p))
    ref.ref_bvh_destroy(h)
    np.savez_compressed(os.path.join(HERE, "trace_zoo.npz"), rays=rays, t=t, prim=prim)
    print("trace_zoo:", n, "rays, hits", int((prim != 0xFFFFFFFF).sum()))

    gen_trace_cwbvh()

    # oracle regression frames
    from unity_webgpu_pathtracer_amd import plugin
    for name, sc, w, hgt, spp, seed in (("cornell", scenes.cornell_box(), 32, 32, 2, 0x12345678),
                                       ("zoo", scenes.material_zoo(), 40, 24, 2, 0xC0FFEE)):
        nodes, tris = plugin.build_cwbvh(sc.vertices)
        b = pyoracle.SceneBuffers(sc, nodes, tris)
        p = scenes.frame_params(sc, w, hgt, spp=spp, seed=seed)
        img, st = pyoracle.render(b, p, threads=1)
        np.savez_compressed(os.path.join(HERE, f"frame_{name}.npz"), frame=img, width=w, height=hgt, spp=spp, seed=seed,
                            stats=np.array([st.as_dict()[k] for k in sorted(st.as_dict())], dtype=np.uint64),
                            stat_names=np.array(sorted(st.as_dict())))
        print(f"frame_{name}: mean {img[..., :3].mean():.5f}")
    # HAS_ENVIRONMENT_TEXTURE regression frame (synthetic HDR lat-long map, scenes.sky_environment)
    sc = scenes.material_zoo(env_map=(64, 32))
    nodes, tris = plugin.build_cwbvh(sc.vertices)
    b = pyoracle.SceneBuffers(sc, nodes, tris)
    w, hgt, spp, seed = 40, 24, 2, 0xE17
    p = scenes.frame_params(sc, w, hgt, spp=spp, seed=seed)
    img, st = pyoracle.render(b, p, threads=1)
    np.savez_compressed(os.path.join(HERE, "frame_zoo_env.npz"), frame=img, width=w, height=hgt, spp=spp, seed=seed, env_w=64, env_h=32,
                        stats=np.array([st.as_dict()[k] for k in sorted(st.as_dict())], dtype=np.uint64),
                        stat_names=np.array(sorted(st.as_dict())))
    print(f"frame_zoo_env: mean {img[..., :3].mean():.5f}")

    # presentation blit and ingestion: regression pins of the restatements (tests/test_present.py, tests/test_ingest.py)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_present
    import test_ingest
    from unity_webgpu_pathtracer_amd import ingest
    f = test_present._hdr_frame(24, 10, seed=3)
    outs = {}
    for i, (mode, srgb, kw) in enumerate(test_present.CASES):
        outs[f"case{i}"] = pyoracle.present(test_present._params(24, 10, mode, srgb, **kw), f)
    np.savez_compressed(os.path.join(HERE, "present_cases.npz"), frame=f, **outs)
    meshes = test_ingest._mesh_zoo()
    descs, total, keep = ingest.mesh_descs(meshes)
    pos, attrs = pyoracle.process_meshes(list(descs), total)
    np.savez_compressed(os.path.join(HERE, "ingest_mesh_zoo.npz"), positions=pos[::7], attrs=attrs.view(np.uint8).reshape(total, 128)[::5],
                        total=total)
    print("present_cases, ingest_mesh_zoo written")


def gen_live_pins():
    """ref_builds.npz, ref_walker_sponza03.npz, ref_cwbvh_walker_sponza03.npz: the reference's outputs for the very inputs
    of the *_live tests, which build them with their own helpers (imported from tests/)."""
    import hashlib
    sys.path.insert(0, os.path.dirname(HERE))
    import test_bvh_builder
    import test_oracle
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    cases, instances = test_bvh_builder._live_cases()
    cw = [pyoracle.ref_build_cwbvh(v) for v in cases]
    tl = [pyoracle.ref_build_tlas(inst) for inst in instances]
    np.savez_compressed(os.path.join(HERE, "ref_builds.npz"), cwbvh_nodes=np.array([sha(n) for n, _ in cw]),
                        cwbvh_tris=np.array([sha(t) for _, t in cw]), tlas_nodes=np.array([sha(n) for n, _ in tl]),
                        tlas_indices=np.array([sha(i) for _, i in tl]))
    s, raw = test_oracle._walker_live_case()
    t, prim = test_oracle._ref_walker_trace(pyoracle.load_ref_tinybvh(), s, raw)
    np.savez_compressed(os.path.join(HERE, "ref_walker_sponza03.npz"), t=t, prim=prim)
    s, raw = test_oracle._cwbvh_walker_live_case()
    records, nodes, tris = pyoracle.ref_cwbvh_trace(s.vertices, raw, threads=4)
    np.savez_compressed(os.path.join(HERE, "ref_cwbvh_walker_sponza03.npz"), records=records, node_sha256=sha(nodes), tri_sha256=sha(tris))
    print("ref_builds, ref_walker_sponza03, ref_cwbvh_walker_sponza03 written")


def gen_helmet_geometry(src):
    """helmet_geometry.npz: the .glb at `src` with every buffer view that no accessor reads (the embedded images) cut to zero
    length; the JSON chunk (nodes, meshes, materials, textures, images) is kept, so load_glb(load_images=False) reads the
    same meshes and materials from it as from the original."""
    import json
    import struct
    from unity_webgpu_pathtracer_amd import ingest
    doc, blob = ingest._glb_chunks(open(src, "rb").read())
    used = {a["bufferView"] for a in doc["accessors"] if "bufferView" in a}
    out = bytearray()
    for i, bv in enumerate(doc["bufferViews"]):
        start, length = bv.get("byteOffset", 0), bv["byteLength"]
        if i in used:
            out += bytes(-len(out) % 4)
            bv["byteOffset"] = len(out)
            out += blob[start:start + length]
        else:
            bv["byteOffset"], bv["byteLength"] = 0, 0
    out += bytes(-len(out) % 4)
    doc["buffers"] = [{"byteLength": len(out)}]
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * (-len(js) % 4)
    glb = struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(js) + 8 + len(out)) + struct.pack("<II", len(js), 0x4E4F534A) + js \
        + struct.pack("<II", len(out), 0x004E4942) + bytes(out)
    np.savez_compressed(os.path.join(HERE, "helmet_geometry.npz"), glb=np.frombuffer(glb, np.uint8))
    print(f"helmet_geometry written ({len(glb)} bytes of .glb)")


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1:3] == ["--only", "helmet"]:
        gen_helmet_geometry(sys.argv[3])
    elif len(sys.argv) > 2 and sys.argv[1] == "--only":       # regenerate one family without touching the others
        pyoracle.build(ref=True)
        {"trace_cwbvh": gen_trace_cwbvh, "live": gen_live_pins}[sys.argv[2]]()
    else:
        main()
