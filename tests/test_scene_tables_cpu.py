"""What brmi_set_scene derives from a scene (basicrenderer_amd/csrc/brmi_scene_tables.h), run on the host under the address and undefined-behaviour
sanitizers: tests/scene_tables_main.cpp is compiled here into a stand-alone program and run as a child process.

  * the tables of generated scenes against a numpy restatement written from the scene's arrays (not from the C++),
  * every refusal: the ones tests/test_parity_gpu.py reaches through the C ABI, with the same message fragments, and the ones no scene generator produces,
  * hand-made hierarchies for the paths where a mesh leaves the flat tables, the spill path and shared pages."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, Scene

LIB = os.path.join(ROOT, "basicrenderer_amd", "lib")
U32_MAX = 0xFFFFFFFF
PAGE_SIZE = 256 * 1024


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_tables") / "scene_tables_main")
    # -static-libasan / -static-libubsan: the sanitizer runtimes are part of the executable, so it does not depend on ASan's check that its shared
    # runtime comes first among the loaded libraries, and nothing has to be put into LD_PRELOAD
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "scene_tables_main.cpp"), "-L" + LIB, "-lbrmi_scene", "-Wl,-rpath," + LIB, "-o", exe])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, f"{args}: exit {r.returncode}\n{r.stderr}"
        return r.stdout

    return run


# ---- the restatement: numpy on the arrays of basicrenderer_amd.Scene (word layouts: include/brmi_types.h) ----
def words(sc, name, n):
    return sc.arrays[name].view(np.uint32).reshape(-1, n)


def expected_tables(sc, boxes_on=True):
    md, nodes, segs, groups = words(sc, "meshMetadata", 10), words(sc, "lodNodes", 16), words(sc, "lodSegments", 4), words(sc, "lodGroups", 19)
    pmap, meshes, insts = words(sc, "groupPageMap", 2), words(sc, "perMesh", 16), words(sc, "perMeshInstance", 8)
    mats, op = words(sc, "materials", 69), words(sc, "openpbrMaterials", 100)
    offs = sc.arrays["clodOffsets"].view(np.uint32)
    e = {}
    # classification
    e["hasCoat"], e["hasFuzz"] = bool((op[:, 24].view(np.float32) > 0).any()), bool((op[:, 34].view(np.float32) > 0).any())
    bind = op[:, 62:]
    slot_on = np.stack([(bind[:, 2 * k] != U32_MAX) & (bind[:, 2 * k + 1] != U32_MAX) for k in range(6)], 1)
    named = list(bind[:, 26:32][slot_on])
    flags = mats[:, 0]
    any_texture = sum(1 << b for b in (1, 2, 3, 4, 6, 7, 12))
    for bit, word in ((9, 58), (1, 52), (2, 53), (6, 54), (7, 55), (4, 56), (3, 57)):      # parallax -> height set; base colour, normal, metallic, roughness, emissive, AO
        named += list(mats[(flags >> bit) & 1 == 1, word])
    e["uvSets"] = 1 + max([int(s) for s in named if s < 8], default=0)
    e["hasTextures"] = bool(slot_on.any() or (flags & any_texture).any())
    e["hasAlphaTest"], e["hasParallax"] = bool((flags >> 13 & 1).any()), bool((flags >> 9 & 1).any())
    e["hasVertexColors"] = bool((meshes[:, 2] & 1).any())
    # hierarchies, level by level: (node, parent position) in breadth-first order
    seg_prefix, mesh_bits, level_width, flat, flat_base = np.zeros(len(segs), np.uint32), [], [], [], []
    e["maxDepth"] = 1
    for m in range(len(md)):
        groups_base, segs_base, nodes_base, root, page_map_base = (int(md[m, w]) for w in (0, 1, 2, 3, 6))
        order, level, widths = [], [(root, 0)], []
        while level:
            widths.append(len(level)); first = len(order); order += level; level = []
            for k, (n, _) in enumerate(order[first:], first):
                nd = nodes[nodes_base + n]
                if nd[0] == 0:
                    level += [(int(nd[1]) + c, k) for c in range(min(int(nd[2]) + 1, 8))]
        leaves = [nodes[nodes_base + n] for n, _ in order if nodes[nodes_base + n][0] != 0]
        count = 1 + max(int(nd[1]) for nd in leaves)
        meshlets = segs[segs_base: segs_base + count, 2].astype(np.uint64)
        seg_prefix[segs_base: segs_base + count] = np.cumsum(meshlets) - meshlets
        mesh_bits.append(int(meshlets.sum())); level_width.append(max(widths)); e["maxDepth"] = max(e["maxDepth"], len(widths))
        assert len(order) <= 8192 and len(widths) <= 64      # (these scenes: every mesh gets flat tables)
        flat_base.append(len(flat))
        for k, (n, parent) in enumerate(order):
            nd = nodes[nodes_base + n]
            kids = [j for j, (_, par) in enumerate(order) if par == k and j != 0]
            rec = dict(nodeId=n, parent=parent, firstChild=kids[0] if kids else 0, childCount=len(kids), spheres=nd[4:13].tobytes(), bits=1, pageMapIndex=0, firstBitRel=0, segFirstCount=0, ownerGroup=0,
                       leaf=np.zeros(12, np.uint32))
            if nd[0] != 0:
                seg = segs[segs_base + int(nd[1])]
                rec.update(bits=(2 if nd[2] else 0) | (4 if seg[2] else 0), pageMapIndex=page_map_base + int(seg[3]), firstBitRel=int(seg_prefix[segs_base + int(nd[1])]), segFirstCount=int(seg[1]) | int(seg[2]) << 16,
                           ownerGroup=int(nd[3]))
                rec["leaf"][0:4] = groups[groups_base + int(nd[3]), 0:4]; rec["leaf"][9] = groups_base + int(nd[3])
                if nd[2]:
                    child = groups_base + int(nd[2]) - 1
                    rec["leaf"][4:8] = groups[child, 0:4]; rec["leaf"][8] = groups[child, 17]; rec["leaf"][10] = child
            flat.append(rec)
    e["flat"], e["segPrefix"], e["meshLevelWidth"] = flat, seg_prefix, np.array(level_width, np.uint32)
    e["flatCountPerMesh"] = np.diff(flat_base + [len(flat)])
    e["maxLevelWidth"], e["minLevelWidth"] = max(level_width), min(level_width)
    bits = np.array(mesh_bits, np.uint64)[offs]
    e["instanceBitBase"], e["totalBits"] = (np.cumsum(bits) - bits).astype(np.uint32), int(bits.sum())
    skinned = (meshes[insts[:, 0], 2] >> 3) & 1
    e["instanceWalk"] = np.stack([np.array(flat_base, np.uint32)[offs], e["flatCountPerMesh"].astype(np.uint32)[offs], e["instanceBitBase"], skinned.astype(np.uint32)], 1)
    # resident pages in page-map order, each once
    box_base, refs, total = np.full(len(sc.slabs) * 1024, U32_MAX, np.uint32), [], 0
    for slab, offset in pmap if boxes_on else []:
        page = int(offset) // PAGE_SIZE
        if slab == 0 or page >= 1024 or sc.slabs[slab] is None or box_base[int(slab) * 1024 + page] != U32_MAX:
            continue
        meshlets = min(int(sc.slabs[slab][int(offset): int(offset) + 4].view(np.uint32)[0]), (PAGE_SIZE - 64) // 64)
        box_base[int(slab) * 1024 + page] = total; refs.append((slab, offset, total, meshlets)); total += meshlets
    e["pageBoxBase"], e["pageRefs"], e["totalBoxes"] = box_base, np.array(refs, np.uint32).reshape(-1, 4), total
    return e


SCENES = {"plain": dict(), "textured": dict(material_features=8), "coat_fuzz": dict(material_features=3), "skinned": dict(skinned_fraction=1.0)}


@pytest.mark.parametrize("name", list(SCENES))
def test_tables_match_a_numpy_restatement(program, tmp_path, name):
    kw = SCENES[name]
    sc = Scene("tiny", 128, 72, point_lights=1, lod_levels=2, **kw)
    total_boxes_off = int(program("tables", tmp_path, kw.get("material_features", 0), int(round(kw.get("skinned_fraction", 0.0) * 1024))))

    def got(file, cols=None):
        a = np.fromfile(os.path.join(str(tmp_path), file), dtype=np.uint32)
        return a.reshape(-1, cols) if cols else a

    with open(os.path.join(str(tmp_path), "scalars.json")) as f:
        s = json.load(f)
    e = expected_tables(sc)
    for key in ("hasCoat", "hasFuzz", "hasAlphaTest", "hasTextures", "hasParallax", "hasVertexColors"):
        assert bool(s[key]) == e[key], key
    for key in ("uvSets", "totalBits", "maxDepth", "maxLevelWidth", "minLevelWidth", "totalBoxes"):
        assert s[key] == e[key], key
    assert np.array_equal(got("segPrefix.u32"), e["segPrefix"])
    assert np.array_equal(got("instanceBitBase.u32"), e["instanceBitBase"])
    assert np.array_equal(got("meshLevelWidth.u32"), e["meshLevelWidth"])
    walk = got("instanceWalk.u32", 4)
    assert np.array_equal(walk, e["instanceWalk"])
    # per mesh, the flat node count (an instance's record names its mesh's): every mesh of these scenes is instanced
    offs = sc.arrays["clodOffsets"].view(np.uint32)
    assert set(offs) == set(range(len(e["flatCountPerMesh"])))
    for i, m in enumerate(offs):
        assert walk[i, 1] == e["flatCountPerMesh"][m]
    assert s["allMeshesFlat"] == 1 and s["anyWideFlat"] == int((e["flatCountPerMesh"] > 256).any()) and s["flatMaxDepth"] == e["maxDepth"] and s["spillLevels"] == 0
    nodes, leaves = got("flatNodes.bin", 16), got("flatLeaves.bin", 12)
    assert len(nodes) == len(leaves) == len(e["flat"]) == s["flatNodes"]
    for k, rec in enumerate(e["flat"]):
        n = nodes[k]
        assert (n[9], n[10] >> 8, n[15] & 0xFFFF, n[15] >> 16, n[10] & 0xFF, n[13], n[14], n[12]) == \
               (rec["nodeId"], rec["parent"], rec["firstChild"], rec["childCount"], rec["bits"], rec["pageMapIndex"], rec["firstBitRel"], rec["segFirstCount"]), k
        assert n[:9].tobytes() == rec["spheres"] and n[11] == rec["ownerGroup"] and np.array_equal(leaves[k], rec["leaf"]), k
    assert np.array_equal(got("pageRefs.u32", 4), e["pageRefs"]) and np.array_equal(got("pageBoxBase.u32"), e["pageBoxBase"]) and len(e["pageRefs"]) > 0
    off = expected_tables(sc, boxes_on=False)
    assert total_boxes_off == off["totalBoxes"] == 0
    assert np.array_equal(got("pageRefs_off.u32", 4), off["pageRefs"]) and np.array_equal(got("pageBoxBase_off.u32"), off["pageBoxBase"])
    if name == "skinned":
        assert walk[:, 3].any()
    if name == "textured":
        assert e["hasTextures"]
    if name == "coat_fuzz":
        assert e["hasCoat"] and e["hasFuzz"]


INVALID, CAPACITY = -1, -3
REFUSALS = [  # (corruption, status, message fragment); the first twelve: test_dangling_scene_indices_are_refused / test_missing_texture_table_is_refused of test_parity_gpu.py
    ("activeDraws", INVALID, "activeDraws"), ("perMeshBufferIndex", INVALID, "perMeshBufferIndex"), ("perObjectBufferIndex", INVALID, "perObjectBufferIndex"),
    ("materialDataIndex", INVALID, "materialDataIndex"), ("slab", INVALID, "slab"), ("pageBoundary", INVALID, "page boundary"), ("segmentPage", INVALID, "page"),
    ("clodOffsets", INVALID, "mesh metadata"), ("leafGroup", INVALID, "names group"), ("leafRefinedGroup", INVALID, "refined group"),
    ("openPBRMaterialDataIndex", INVALID, "openPBRMaterialDataIndex"), ("textureTable", INVALID, "texture"),
    ("nodeOutOfRange", INVALID, "mesh 0: node 1001 out of range"), ("segmentOutOfRange", INVALID, "mesh 0: segment 1 out of range"),
    ("segmentWraps", INVALID, "mesh 0: leaf node 2 names segment 4294967295, which does not exist"), ("deeperThan64", INVALID, "mesh 0: BVH deeper than 64 levels"),
    ("skinningSlot", INVALID, "mesh instance 0: skinning slot 3 lies outside the skinning matrix buffer"), ("openpbrRecords", CAPACITY, "65537 OpenPBR material records"),
    ("meshMeshlets", CAPACITY, "mesh 0 has too many meshlets"), ("instancePairs", CAPACITY, "scene exceeds 2^32 (instance, meshlet) pairs")]


@pytest.mark.parametrize("corruption,status,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(program, corruption, status, fragment):
    code, message = program("refuse", corruption).split("\n", 1)
    assert int(code) == status and fragment in message, message


def test_fallbacks_on_hand_made_hierarchies(program):
    def shape(name):
        return json.loads(program("shape", name))

    plain = shape("plain")                  # a root and two leaves of one 4-meshlet segment in one page
    assert (plain["flatCounts"], plain["flatNodes"], plain["allMeshesFlat"], plain["pageRefs"], plain["totalBoxes"], plain["totalBits"]) == ([3], 3, 1, 1, 4, 4)
    big = shape("tooManyNodes")             # a complete 8-ary tree of 6 levels, 37449 nodes: more than the 8192 a flat table takes
    assert big["flatCounts"] == [0] and big["allMeshesFlat"] == 0 and big["flatNodes"] == 0
    assert big["maxLevelWidth"] == 8 ** 5 and big["spillLevels"] == 6 - 4 + 1      # depth less the first level of more than 128 nodes (the fourth: 512), plus one
    wide = shape("wideLevel")               # 5 levels, 4681 nodes: flat, and wider than the 1024 nodes of the LDS walk
    assert wide["flatCounts"] == [4681] and wide["allMeshesFlat"] == 1 and wide["anyWideFlat"] == 1 and wide["flatMaxDepth"] == 5
    assert wide["maxLevelWidth"] == 8 ** 4 and wide["spillLevels"] == 5 - 4 + 1
    seg = shape("bigSegment")               # a second mesh whose second node is a leaf of a 65536-meshlet segment: its root's record is taken back
    assert seg["flatCounts"] == [3, 0] and seg["flatNodes"] == seg["flatLeaves"] == 3 and seg["allMeshesFlat"] == 0
    deep = shape("deepForLevelBound")       # 4 levels under maxBvhLevels = 3
    assert deep["flatCounts"] == [0] and deep["allMeshesFlat"] == 0 and deep["maxDepth"] == 4 and deep["flatMaxDepth"] == 1
    fits = shape("deepWithinLevelBound")    # ... and under maxBvhLevels = 4
    assert fits["flatCounts"] == [4] and fits["allMeshesFlat"] == 1 and fits["flatMaxDepth"] == 4
    shared = shape("sharedPage")            # page-map entries: page 0 of slab 1 twice, its page 1 (7 meshlets), a non-resident one
    assert shared["pageRefs"] == 2 and shared["totalBoxes"] == 4 + 7
