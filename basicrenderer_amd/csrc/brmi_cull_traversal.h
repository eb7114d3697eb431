// brmi_cull_traversal.h -- the traversal and cluster-cull kernels (K2, K1 + K2, K3) of brmi_cull.hip.
// Included TWICE by brmi_cull.hip: BRMI_STREAMING_PASS 0 gives the kernels under their own names, every group resident (the code they always were);
// BRMI_STREAMING_PASS 1 gives `<name>_streaming` with a trailing StreamArgs argument and the residency rule (brmi_set_streaming).  The branches are
// `if constexpr` on the macro: the pass without streaming discards them before code generation.
#if BRMI_STREAMING_PASS
#define BRMI_CULL_KERNEL(name) name##_streaming
#define BRMI_ST_PARAM , StreamArgs st
#define BRMI_ST_ARG st
#else
#define BRMI_CULL_KERNEL(name) name
#define BRMI_ST_PARAM
#define BRMI_ST_ARG StreamArgs{}
#endif

// K2: one BFS level ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) BRMI_CULL_KERNEL(k_traverse)(CullArgs a, uint32_t level, const NodeRecord* frontierIn, NodeRecord* frontierOut, BucketRecord* buckets BRMI_ST_PARAM) {
    const brmi_scene_buffers& sc = a.sc;
    const uint32_t inputCount = min(a.counters[level == 0 ? a.frontier0Counter : CNT_FRONTIER0 + level], a.recordCapacity);
    const uint32_t viewId = sc.perFrame->mainCameraIndex;
    const brmi_camera* cam = sc.cameras + viewId;
    const brmi_culling_camera* lodCam = sc.cullingCameras + viewId;
    const bool ortho = cam->isOrtho != 0;
    const f3 camPos{lodCam->positionWorldSpace[0], lodCam->positionWorldSpace[1], lodCam->positionWorldSpace[2]};
    const float zNear = lodCam->zNear, threshold = lodCam->errorOverDistanceThreshold;
    const m4 view = load_m4(&cam->view[0][0]);
    uint32_t* nextCount = &a.counters[CNT_FRONTIER0 + level + 1];
    const uint32_t rounded = (inputCount + 63u) & ~63u;
    for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < rounded; idx += gridDim.x * blockDim.x) {
        bool have = idx < inputCount;
        // phase 2 of a mixed traversal: the replay buffer also holds nodes of the narrow instances, which k_cull_hierarchy<true> walks
        if (have && level == 0u && a.phase == 2u && a.levelKernelsWidthLo != 0u &&
            a.meshLevelWidth[sc.clodOffsets[frontierIn[idx].instanceIndex].clodMeshMetadataIndex] < a.levelKernelsWidthLo) have = false;
        // per-record state
        bool isInternal = false, emitLeaf = false, replay = false, occluded = false;
        uint32_t occludedNode = 0;
        uint32_t instIndex = 0, childBase = 0, childCount = 0, lodNodesBase = 0;
        uint32_t segFirst = 0, segCount = 0, ownerGroup = 0, slabDesc = 0, slabOff = 0, firstBit = 0;
        bool skinned = false;
        m4 model{}; float scale = 0.0f;
        f3 instC{0, 0, 0}; float instR = 0.0f;
        if (have) {
            const NodeRecord rec = frontierIn[idx];
            instIndex = rec.instanceIndex;
            replay = (rec.nodeIdPacked >> 31) != 0;
            const bool allowRefine = ((rec.nodeIdPacked >> 30) & 1u) != 0;
            const uint32_t nodeId = rec.nodeIdPacked & 0x3FFFFFFFu;
            const brmi_per_mesh_instance inst = sc.perMeshInstance[instIndex];
            const brmi_clod_mesh_metadata md = sc.meshMetadata[sc.clodOffsets[instIndex].clodMeshMetadataIndex];
            skinned = (sc.perMesh[inst.perMeshBufferIndex].vertexFlags & BRMI_VERTEX_SKINNED) != 0;
            model = load_m4(&sc.perObject[inst.perObjectBufferIndex].model[0][0]);
            scale = max_axis_scale(model);
            instC = f3{inst.boundingSphere[0], inst.boundingSphere[1], inst.boundingSphere[2]}; instR = inst.boundingSphere[3];
            lodNodesBase = md.lodNodesBase;
            const brmi_lod_node node = sc.lodNodes[md.lodNodesBase + nodeId];
            const f3 cullC = skinned ? instC : f3{node.cullCenterAndRadius[0], node.cullCenterAndRadius[1], node.cullCenterAndRadius[2]};
            const float cullR = skinned ? instR : node.cullCenterAndRadius[3];
            const f3 cVS = to_view_space(cullC, model, view);
            const float rW = cullR * scale;
            const bool culled = !replay && sphere_culled(a, cam, cVS, rW);
            if (!culled) {
                if (node.isLeaf != BRMI_NODE_INTERNAL) {
                    const brmi_lod_group* g = sc.lodGroups + (md.groupsBase + node.ownerGroupId);
                    const f3 gc = xyz(mul_point(f3{g->centerAndRadius[0], g->centerAndRadius[1], g->centerAndRadius[2]}, model));
                    const float gr = g->centerAndRadius[3] * scale;
                    const float eod = projected_error(gc, gr, node.maxQuadricError, scale, camPos, zNear, ortho);
                    bool ok = allowRefine && (eod >= threshold);
                    if constexpr (BRMI_STREAMING_PASS) {      // owner touched behind wantsRender, refined child only when its boundary error holds, leaf dropped when its own group is missing
                        if (ok) {
                            const bool canRender = stream_touch(BRMI_ST_ARG, md.groupsBase + node.ownerGroupId, instIndex, eod);
                            if (node.countMinusOne != 0u && !(refined_child_eod(sc, md.groupsBase + node.countMinusOne - 1u, model, scale, camPos, zNear, ortho) < threshold) &&
                                stream_touch(BRMI_ST_ARG, md.groupsBase + node.countMinusOne - 1u, instIndex, eod)) ok = false;
                            if (!canRender) ok = false;
                        }
                    } else
                    if (ok && refined_child_suppresses(sc, md.groupsBase, node.countMinusOne - 1u, node.countMinusOne != 0u, model, scale, camPos, zNear, threshold, ortho)) ok = false;
                    if (ok) {
                        const brmi_lod_segment seg = sc.lodSegments[md.segmentsBase + node.indexOrOffset];
                        const brmi_group_page_map_entry pe = sc.groupPageMap[md.pageMapBase + seg.pageIndex];
                        if (seg.meshletCount != 0u && pe.slabDescriptorIndex != 0u) {
                            emitLeaf = true;
                            segFirst = seg.firstMeshletInPage; segCount = seg.meshletCount; ownerGroup = node.ownerGroupId;
                            slabDesc = pe.slabDescriptorIndex; slabOff = pe.slabByteOffset;
                            firstBit = a.instanceBitBase[instIndex] + a.segPrefix[md.segmentsBase + node.indexOrOffset];
                        }
                    }
                } else {
                    const f3 lc = xyz(mul_point(f3{node.lodCenterAndRadius[0], node.lodCenterAndRadius[1], node.lodCenterAndRadius[2]}, model));
                    const float lr = node.lodCenterAndRadius[3] * scale;
                    const float nodeEod = projected_error(lc, lr, node.maxQuadricError, scale, camPos, zNear, ortho);
                    if (allowRefine && (nodeEod >= threshold)) {
                        if (a.occlusion && occlusion_test(a, cam, replay, cullC, cullR, cVS, rW, sc.perObject + inst.perObjectBufferIndex)) {
                            occluded = !replay; occludedNode = nodeId;     // a node rejected in phase 2 is simply dropped
                        } else {
                            isInternal = true;
                            childBase = node.indexOrOffset;
                            childCount = min(node.countMinusOne + 1u, BRMI_BVH_MAX_CHILDREN);
                        }
                    }
                }
            }
        }
        {   // statistics: one atomic per wave on one of 64 stripes
            const uint64_t hm = __ballot(have);
            if (hm != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(&a.counters[CNT_STRIPES + (blockIdx.x & (CNT_STRIPE_COUNT - 1u)) * CNT_STRIPE_WORDS + 2u], (uint32_t)__popcll(hm));
        }
        if (a.occlusion && a.phase == 1u) {   // hand the rejected node to phase 2 (workGraphCulling.hlsl:3094-3112: drop + count when full)
            const uint32_t slot = wave_append(&a.counters[CNT_REPLAY_NODES], occluded);
            if (occluded) {
                if (slot < a.recordCapacity) a.replayNodes[slot] = NodeRecord{instIndex, 0x80000000u | (1u << 30) | (occludedNode & 0x3FFFFFFFu)};
                else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
            }
        }
        // leaf: chunk the segment into bucket records of `factor` meshlets (computeCulling.hlsl:385-406)
        // wave-cooperative emission: iterate chunk index k over the widest leaf in the wave
        {
            const uint32_t nChunks = emitLeaf ? (segCount + a.factor - 1u) / a.factor : 0u;
            uint32_t waveMax = nChunks;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) waveMax = max(waveMax, (uint32_t)__shfl_xor((int)waveMax, o));
            for (uint32_t k = 0; k < waveMax; k++) {
                const bool emit = k < nChunks;
                const uint32_t slot = wave_append(&a.counters[a.bucketCounter], emit);
                if (emit) {
                    if (slot < a.recordCapacity) {
                        const uint32_t first = segFirst + k * a.factor;
                        const uint32_t cnt = min(a.factor, segCount - k * a.factor);
                        BucketRecord b;
                        b.instanceIndex = instIndex; b.groupIdPacked = (replay ? 0x80000000u : 0u) | (ownerGroup & 0x7FFFFFFFu);
                        b.meshletIndexAndCount = (cnt << 16) | (first & 0xFFFFu);
                        b.pageSlabDescriptorIndex = slabDesc; b.pageSlabByteOffset = slabOff;
                        b.firstBit = firstBit + k * a.factor; b.pad0 = 0; b.pad1 = 0;
                        buckets[slot] = b;
                    } else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
                }
            }
        }
        // internal: pre-filter children, append survivors to the next frontier (computeCulling.hlsl:477-530)
        {
            uint32_t waveMax = isInternal ? childCount : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) waveMax = max(waveMax, (uint32_t)__shfl_xor((int)waveMax, o));
            for (uint32_t k = 0; k < waveMax; k++) {
                bool emit = false;
                uint32_t childId = 0;
                if (isInternal && k < childCount) {
                    childId = childBase + k;
                    const brmi_lod_node* ch = sc.lodNodes + (lodNodesBase + childId);
                    const f3 cc = skinned ? instC : f3{ch->cullCenterAndRadius[0], ch->cullCenterAndRadius[1], ch->cullCenterAndRadius[2]};
                    const float cr = skinned ? instR : ch->cullCenterAndRadius[3];
                    const f3 ccVS = to_view_space(cc, model, view);
                    emit = replay || !sphere_culled(a, cam, ccVS, cr * scale);
                    if (emit && ch->isLeaf == BRMI_NODE_INTERNAL) {
                        const f3 wc = xyz(mul_point(f3{ch->lodCenterAndRadius[0], ch->lodCenterAndRadius[1], ch->lodCenterAndRadius[2]}, model));
                        const float e = projected_error(wc, ch->lodCenterAndRadius[3] * scale, ch->maxQuadricError, scale, camPos, zNear, ortho);
                        if (e < threshold) emit = false;
                    }
                }
                const uint32_t slot = wave_append(nextCount, emit);
                if (emit) {
                    if (slot < a.recordCapacity) frontierOut[slot] = NodeRecord{instIndex, (replay ? 0x80000000u : 0u) | (1u << 30) | (childId & 0x3FFFFFFFu)};
                    else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
                }
            }
        }
    }
}

// K1 + K2 in one launch: one wave64 per draw (phase 1) or per replayed node (phase 2) walks that instance's BVH breadth-first
// with the frontier in LDS.  Instances are independent, so the level-by-level kernel sequence above -- one launch and ~8
// dependent HBM round trips per level for every instance -- becomes one launch in which the per-instance state (instance,
// mesh metadata, model matrix) is fetched once and a level costs node -> group / segment -> page map.  Used when every mesh's
// BVH level fits the LDS frontier (brmi_set_scene checks); same tests, same operation order as k_cull_instances / k_traverse.
// HIER_CAP nodes per frontier, HIER_STAGE bucket records staged in LDS: (256, 128) = 6 KB keeps ~20 workgroups per CU in flight
// (scenes of many small instances), (1024, 128) = 12 KB covers wide hierarchies.  Meshes wider than that (a street's ground and facades
// tessellated to pixel-sized triangles: 1,600 leaf segments on one level) go through the level-per-launch kernels, which put every
// lane of the chip on one level -- a single wave walking such a mesh alone took 0.4 ms (tried with a 4096-node variant).
// SIDE (brmi_execute, phase 1): the launch carries extra workgroups behind the traversal's that clear the visibility buffer.  The walk is a
// chain of dependent loads on ~1.3 waves per SIMD; the 66 MB of stores disappear in its shadow instead of costing a launch of their own.
// Behind those, one workgroup per light cluster runs the first half of the light clustering (AABB + hit masks + page demand: it depends on
// the frame constants alone); the second half rides on k_cull_clusters.  Frame: three launches and ~25 us less.
template <bool REPLAY, uint32_t HIER_CAP, uint32_t HIER_STAGE, bool SIDE = false>
// Spill mode (meshes wider than `spillAbove` nodes per level): the walk keeps such an instance only while its frontier is small enough for the
// next level to fit the LDS frontier whatever the fan-out (<= HIER_CAP / 8 nodes) and then appends the frontier to `spillOut`, the level-0 input
// of the level kernels.  The top levels of a wide hierarchy hold a handful of nodes each; as level launches they cost 12 us apiece.
__global__ void __launch_bounds__(64) BRMI_CULL_KERNEL(k_cull_hierarchy)(CullArgs a, BucketRecord* buckets, const uint32_t* meshLevelWidth, uint32_t widthLo, uint32_t widthHi, uint32_t spillAbove, NodeRecord* spillOut,
                                                    typename std::conditional<SIDE, SideJobs, NoSide>::type sj BRMI_ST_PARAM) {
    uint32_t walkBlocks = gridDim.x;
    if constexpr (SIDE) {
        walkBlocks = sj.walkBlocks;
        if (blockIdx.x >= sj.walkBlocks + sj.clearBlocks) { lc_count_wave(sj.lc, blockIdx.x - sj.walkBlocks - sj.clearBlocks, threadIdx.x); return; }
        if (blockIdx.x >= sj.walkBlocks) {
            const uint64_t stride = (uint64_t)sj.clearBlocks * 64u;
            for (uint64_t i = (uint64_t)(blockIdx.x - sj.walkBlocks) * 64u + threadIdx.x; i < sj.n2; i += stride) sj.vis2[i] = make_ulonglong2(BRMI_VIS_EMPTY, BRMI_VIS_EMPTY);
            return;
        }
    }
    __shared__ uint32_t frontier[2][HIER_CAP];
    __shared__ uint32_t counts[2];
    __shared__ uint32_t childOff[65], childFirst[64];
    __shared__ BucketRecord stage[HIER_STAGE];     // bucket records of the instance being walked: one global reservation per flush
    const brmi_scene_buffers& sc = a.sc;
    const uint32_t lane = threadIdx.x;
    const uint32_t viewId = sc.perFrame->mainCameraIndex;
    const brmi_camera* cam = sc.cameras + viewId;
    const brmi_culling_camera* lodCam = sc.cullingCameras + viewId;
    const bool ortho = cam->isOrtho != 0;
    const f3 camPos{lodCam->positionWorldSpace[0], lodCam->positionWorldSpace[1], lodCam->positionWorldSpace[2]};
    const float zNear = lodCam->zNear, threshold = lodCam->errorOverDistanceThreshold;
    const m4 view = load_m4(&cam->view[0][0]);
    const uint32_t seeds = REPLAY ? min(a.counters[CNT_REPLAY_NODES], a.recordCapacity) : sc.activeDrawCount;
    uint32_t nTested = 0, nVisible = 0, nNodes = 0;
    uint32_t staged = 0;                            // wave-uniform
    auto flush = [&]() {
        if (staged == 0u) return;
        uint32_t baseSlot = 0;
        if (lane == 0) baseSlot = atomicAdd(&a.counters[a.bucketCounter], staged);
        baseSlot = (uint32_t)__shfl((int)baseSlot, 0);
        __syncthreads();
        for (uint32_t k = lane; k < staged; k += 64u) {
            if (baseSlot + k < a.recordCapacity) buckets[baseSlot + k] = stage[k];
            else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
        }
        __syncthreads();
        staged = 0u;
    };
    // ---- eight instances to a wave.  The typical hierarchy of these scenes has five nodes (median; 90 % have <= 9): a wave per instance leaves
    // 59 lanes idle AND queues two atomics with return per instance on two counters that serve ~90 per microsecond (2,017 instances: 19 us
    // for the last wave, the launch's length).  The first ceil(draws / 8) waves take eight consecutive draws each, eight lanes per draw --
    // object matrices per lane --, evaluate those whose hierarchy has <= 8 nodes exactly as the one-instance path below does, and make ONE
    // reservation per counter for all of them; the waves behind them take one draw each and skip what was handled here.
    uint32_t firstSeed = blockIdx.x, seedStride = walkBlocks;
    if (!REPLAY && a.packedFlat) {
        const uint32_t packedWaves = (seeds + 7u) >> 3;
        if (blockIdx.x < packedWaves) {
            const uint32_t g8 = lane & ~7u, j = lane & 7u;
            const uint32_t seed = blockIdx.x * 8u + (lane >> 3);
            const bool haveSeed = seed < seeds;
            const uint32_t instIndex = haveSeed ? sc.activeDraws[seed] : 0u;
            brmi_per_mesh_instance inst{}; InstanceWalk iw{0u, 0u, 0u, 0u};
            if (haveSeed) { inst = sc.perMeshInstance[instIndex]; iw = a.instanceWalk[instIndex]; }
            const bool small = haveSeed && iw.flatCount >= 1u && iw.flatCount <= 8u;
            const brmi_per_object* obj = sc.perObject + (small ? inst.perObjectBufferIndex : 0u);
            const bool mine = small && j < iw.flatCount;
            FlatNode fn{}; FlatLeaf fl{};
            if (mine) { fn = a.flatNodes[iw.flatBase + j]; fl = a.flatLeaves[iw.flatBase + j]; }
            m4 model = load_m4(&obj->model[0][0]);
            m4 prevModel = model;
            if (a.occlusion && mine && ((fn.info & 1u))) prevModel = load_m4(&obj->prevModel[0][0]);       // (internal nodes: the occlusion test's matrix, requested now)
            const float scale = max_axis_scale(model);
            const f3 instC{inst.boundingSphere[0], inst.boundingSphere[1], inst.boundingSphere[2]}; const float instR = inst.boundingSphere[3];
            bool instVisible = false;
            {   // K1 (PureComputeObjectCullCS), by every lane of the draw's group alike
                const f3 c = to_view_space(instC, model, view);
                const float r = instR * scale;
                const bool bad = isnan(c.x) || isnan(c.y) || isnan(c.z) || isinf(c.x) || isinf(c.y) || isinf(c.z) || isnan(r) || isinf(r);
                instVisible = small && !bad && !sphere_culled(a, cam, c, r);
            }
            nTested += (uint32_t)__popcll(__ballot(small && j == 0u)); nVisible += (uint32_t)__popcll(__ballot(instVisible && j == 0u));
            const bool skinned = iw.skinned != 0u;
            const bool internal = (fn.info & 1u);
            const f3 cullC = skinned ? instC : f3{fn.cull[0], fn.cull[1], fn.cull[2]};
            const float cullR = skinned ? instR : fn.cull[3];
            const f3 cVS = to_view_space(cullC, model, view);
            const float rW = cullR * scale;
            const bool inFrustum = mine && instVisible && !sphere_culled(a, cam, cVS, rW);
            bool pre = inFrustum, expand = false, hidden = false, leafOk = false;
            uint32_t slabDesc = 0, slabOff = 0;
            if (inFrustum && internal) {
                const f3 lc = xyz(mul_point(f3{fn.lod[0], fn.lod[1], fn.lod[2]}, model));
                const float e = projected_error(lc, fn.lod[3] * scale, fn.maxQuadricError, scale, camPos, zNear, ortho);
                pre = e >= threshold;
                if (pre) { hidden = a.occlusion && occlusion_test_prev(a, cam, cullC, cullR, prevModel); expand = !hidden; }
            } else if (inFrustum) {
                const f3 gc = xyz(mul_point(f3{fl.group[0], fl.group[1], fl.group[2]}, model));
                const float eod = projected_error(gc, fl.group[3] * scale, fn.maxQuadricError, scale, camPos, zNear, ortho);
                bool ok = eod >= threshold;
                if (ok && ((fn.info >> 1) & 1u)) {      // refined_child_suppresses
                    const f3 cc = xyz(mul_point(f3{fl.child[0], fl.child[1], fl.child[2]}, model));
                    const float ce = projected_error(cc, fl.child[3] * scale, fl.childParentError, scale, camPos, zNear, ortho);
                    if (!(ce < threshold)) {
                        if constexpr (BRMI_STREAMING_PASS) { if (stream_resident(BRMI_ST_ARG, fl.childGlobal)) ok = false; } else ok = false;
                    }
                }
                if constexpr (BRMI_STREAMING_PASS) { if (ok && !stream_resident(BRMI_ST_ARG, fl.ownerGlobal)) ok = false; }
                if (ok && ((fn.info >> 2) & 1u)) {
                    const brmi_group_page_map_entry pe = sc.groupPageMap[fn.pageMapIndex];
                    slabDesc = pe.slabDescriptorIndex; slabOff = pe.slabByteOffset;
                    leafOk = slabDesc != 0u;
                }
            }
            const uint64_t expandM = __ballot(expand);
            const uint32_t parentLane = g8 | ((fn.info >> 8) & 7u);
            uint64_t reached = __ballot(mine && instVisible && j == 0u);
            for (;;) {
                const bool r = mine && instVisible && (j == 0u || (pre && ((reached >> parentLane) & 1ull) && ((expandM >> parentLane) & 1ull)));
                const uint64_t next = __ballot(r);
                if (next == reached) break;
                reached = next;
            }
            const bool here = (reached >> lane) & 1ull;
            nNodes += here ? 1u : 0u;
            if constexpr (BRMI_STREAMING_PASS) { if (here && inFrustum && !internal) flat_leaf_touch(BRMI_ST_ARG, fn, fl, instIndex, model, scale, camPos, zNear, threshold, ortho); }
            const bool replayIt = a.occlusion && here && hidden;
            const uint64_t replayM = __ballot(replayIt);
            const bool emitLeaf = here && leafOk;
            const uint32_t segFirst = fn.segFirstCount & 0xFFFFu, segCount = fn.segFirstCount >> 16;
            const uint32_t nChunks = emitLeaf ? (segCount + a.factor - 1u) / a.factor : 0u;
            uint32_t incl = nChunks;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, o); if (lane >= (uint32_t)o) incl += v; }
            const uint32_t nBuckets = (uint32_t)__shfl((int)incl, 63), nReplay = (uint32_t)__popcll(replayM);
            uint32_t replayBase = 0, bucketBase = 0;
            if (lane == 0) {
                if (nReplay != 0u) replayBase = atomicAdd(&a.counters[CNT_REPLAY_NODES], nReplay);
                if (nBuckets != 0u) bucketBase = atomicAdd(&a.counters[a.bucketCounter], nBuckets);
            }
            replayBase = (uint32_t)__shfl((int)replayBase, 0); bucketBase = (uint32_t)__shfl((int)bucketBase, 0);
            if (replayIt) {
                const uint32_t slot = replayBase + (uint32_t)__popcll(replayM & ((1ull << lane) - 1ull));
                if (slot < a.recordCapacity) a.replayNodes[slot] = NodeRecord{instIndex, 0x80000000u | (1u << 30) | (fn.nodeId & 0x3FFFFFFFu)};
                else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
            }
            for (uint32_t k = 0; k < nChunks; k++) {
                const uint32_t slot = bucketBase + (incl - nChunks) + k;
                if (slot >= a.recordCapacity) { atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u); continue; }
                BucketRecord b;
                b.instanceIndex = instIndex; b.groupIdPacked = fn.ownerGroup & 0x7FFFFFFFu;
                b.meshletIndexAndCount = (min(a.factor, segCount - k * a.factor) << 16) | ((segFirst + k * a.factor) & 0xFFFFu);
                b.pageSlabDescriptorIndex = slabDesc; b.pageSlabByteOffset = slabOff;
                b.firstBit = iw.bitBase + fn.firstBitRel + k * a.factor; b.pad0 = 0; b.pad1 = 0;
                buckets[slot] = b;
            }
            firstSeed = seeds;                                  // nothing else for this wave
        } else { firstSeed = blockIdx.x - packedWaves; seedStride = walkBlocks - packedWaves; }
    }
    for (uint32_t seed = firstSeed; seed < seeds; seed += seedStride) {
        uint32_t instIndex, startNode;
        if (REPLAY) { const NodeRecord rec = a.replayNodes[seed]; instIndex = rec.instanceIndex; startNode = rec.nodeIdPacked & 0x3FFFFFFFu; }
        else instIndex = sc.activeDraws[seed];
        const brmi_per_mesh_instance inst = sc.perMeshInstance[instIndex];
        if (!REPLAY) {
            // ---- a hierarchy of at most 64 nodes: all of it at once, one lane per node.  The level walk below is a chain of ~10 dependent
            // memory round trips per instance (instance -> mesh metadata -> root -> occlusion -> children -> group / segment -> page map ->
            // bucket slots) and the launch lasts as long as one such chain; here the nodes, the leaves' groups and segments (FlatNode /
            // FlatLeaf, folded by brmi_set_scene) and the object arrive together, the depth chain and the page map together after them.
            // Same tests, same arithmetic, same records; a node is reached iff every ancestor let its children through.
            const InstanceWalk iw = a.instanceWalk[instIndex];
            if (a.packedFlat && iw.flatCount >= 1u && iw.flatCount <= 8u) continue;      // one of the eight draws of a packed wave
            if (iw.flatCount > 256u && a.wideFlat) continue;      // k_cull_flat_wide's
            if (iw.flatCount != 0u && iw.flatCount <= 256u) {
                constexpr uint32_t FLAT_CHUNKS = 4;      // 64 nodes each (brmi_set_scene: hierarchies of up to 256 nodes)
                const uint32_t chunks = (iw.flatCount + 63u) >> 6;
                const brmi_per_object* obj = sc.perObject + inst.perObjectBufferIndex;
                // (what the later phases need of a node; the spheres are used at once)
                uint32_t nodeIdA[FLAT_CHUNKS] = {}, parentA[FLAT_CHUNKS] = {}, ownerGroupA[FLAT_CHUNKS] = {}, segFirstCountA[FLAT_CHUNKS] = {}, firstBitRelA[FLAT_CHUNKS] = {};
                const m4 model = load_m4(&obj->model[0][0]);
                const m4 prevModel = a.occlusion ? load_m4(&obj->prevModel[0][0]) : model;      // (the occlusion test's matrix, requested with the current one)
                const float scale = max_axis_scale(model);
                const f3 instC{inst.boundingSphere[0], inst.boundingSphere[1], inst.boundingSphere[2]}; const float instR = inst.boundingSphere[3];
                {   // K1 (PureComputeObjectCullCS)
                    const f3 c = to_view_space(instC, model, view);
                    const float r = instR * scale;
                    const bool bad = isnan(c.x) || isnan(c.y) || isnan(c.z) || isinf(c.x) || isinf(c.y) || isinf(c.z) || isnan(r) || isinf(r);
                    nTested++;
                    if (bad || sphere_culled(a, cam, c, r)) continue;
                    nVisible++;
                }
                const bool skinned = iw.skinned != 0u;
                uint64_t preM[FLAT_CHUNKS] = {}, expandM[FLAT_CHUNKS] = {}, hiddenM[FLAT_CHUNKS] = {}, leafM[FLAT_CHUNKS] = {}, reached[FLAT_CHUNKS] = {};
                uint32_t slabDescA[FLAT_CHUNKS] = {}, slabOffA[FLAT_CHUNKS] = {};
                [[maybe_unused]] uint64_t seenLeafM[FLAT_CHUNKS] = {};      // (streaming: leaves that reached their error test; touched once they are known to be reached)
#pragma unroll
                for (uint32_t c = 0; c < FLAT_CHUNKS; c++) if (c < chunks) {
                    const bool mine = c * 64u + lane < iw.flatCount;
                    FlatNode fn{}; FlatLeaf fl{};
                    if (mine) { fn = a.flatNodes[iw.flatBase + c * 64u + lane]; fl = a.flatLeaves[iw.flatBase + c * 64u + lane]; }
                    nodeIdA[c] = fn.nodeId; parentA[c] = fn.info >> 8; ownerGroupA[c] = fn.ownerGroup; segFirstCountA[c] = fn.segFirstCount; firstBitRelA[c] = fn.firstBitRel;
                    const bool internal = (fn.info & 1u);
                    const f3 cullC = skinned ? instC : f3{fn.cull[0], fn.cull[1], fn.cull[2]};
                    const float cullR = skinned ? instR : fn.cull[3];
                    const f3 cVS = to_view_space(cullC, model, view);
                    const float rW = cullR * scale;
                    const bool inFrustum = mine && !sphere_culled(a, cam, cVS, rW);
                    // internal node: children pass when its projected error is above the threshold and the depth chain does not hide it;
                    // as a child it was let through on the same two conditions (frustum, error)
                    bool pre = inFrustum, expand = false, hidden = false, leafOk = false;
                    if (inFrustum && internal) {
                        const f3 lc = xyz(mul_point(f3{fn.lod[0], fn.lod[1], fn.lod[2]}, model));
                        const float e = projected_error(lc, fn.lod[3] * scale, fn.maxQuadricError, scale, camPos, zNear, ortho);
                        pre = e >= threshold;
                        if (pre) { hidden = a.occlusion && occlusion_test_prev(a, cam, cullC, cullR, prevModel); expand = !hidden; }
                    } else if (inFrustum) {
                        const f3 gc = xyz(mul_point(f3{fl.group[0], fl.group[1], fl.group[2]}, model));
                        const float eod = projected_error(gc, fl.group[3] * scale, fn.maxQuadricError, scale, camPos, zNear, ortho);
                        bool ok = eod >= threshold;
                        if (ok && ((fn.info >> 1) & 1u)) {      // refined_child_suppresses
                            const f3 cc = xyz(mul_point(f3{fl.child[0], fl.child[1], fl.child[2]}, model));
                            const float ce = projected_error(cc, fl.child[3] * scale, fl.childParentError, scale, camPos, zNear, ortho);
                            if (!(ce < threshold)) {
                                if constexpr (BRMI_STREAMING_PASS) { if (stream_resident(BRMI_ST_ARG, fl.childGlobal)) ok = false; } else ok = false;
                            }
                        }
                        if constexpr (BRMI_STREAMING_PASS) { if (ok && !stream_resident(BRMI_ST_ARG, fl.ownerGlobal)) ok = false; }
                        if (ok && ((fn.info >> 2) & 1u)) {
                            const brmi_group_page_map_entry pe = sc.groupPageMap[fn.pageMapIndex];
                            slabDescA[c] = pe.slabDescriptorIndex; slabOffA[c] = pe.slabByteOffset;
                            leafOk = slabDescA[c] != 0u;
                        }
                    }
                    preM[c] = __ballot(pre); expandM[c] = __ballot(expand); hiddenM[c] = __ballot(hidden); leafM[c] = __ballot(leafOk);
                    if constexpr (BRMI_STREAMING_PASS) seenLeafM[c] = __ballot(inFrustum && !internal);
                }
                // reached: the root, or a node that passed as a child of a reached node that lets its children through
                reached[0] = 1ull;
                for (bool changed = true; changed; ) {
                    changed = false;
#pragma unroll
                    for (uint32_t c = 0; c < FLAT_CHUNKS; c++) if (c < chunks) {
                        const uint32_t parent = parentA[c], pc = parent >> 6, pb = parent & 63u;
                        uint64_t through = 0;      // reached parents that let their children through, the parent's chunk
#pragma unroll
                        for (uint32_t q = 0; q < FLAT_CHUNKS; q++) if (q == pc) through = reached[q] & expandM[q];
                        const bool r = (c == 0u && lane == 0u) || (c * 64u + lane < iw.flatCount && ((preM[c] >> lane) & 1ull) && ((through >> pb) & 1ull) && !(c == 0u && lane == 0u));
                        const uint64_t next = __ballot(r);
                        if (next != reached[c]) { reached[c] = next; changed = true; }
                    }
                }
                // Two reservations per instance -- replay nodes, bucket records -- and every wave of the launch reaches them at about the same
                // time: ~2,000 atomics with return on each counter are served at ~90 per microsecond, 19 us for the last wave, and one after
                // the other they were most of this kernel.  Both are requested back to back (two queues drain side by side), and the
                // records go straight to the bucket array (the LDS stage collects the level walk's records: one instance per wave has
                // nothing to collect).
                uint32_t nReplay = 0, nBuckets = 0;                 // wave totals
                uint32_t replayRank[FLAT_CHUNKS] = {}, bucketRank[FLAT_CHUNKS] = {}, chunksOfLeaf[FLAT_CHUNKS] = {};
#pragma unroll
                for (uint32_t c = 0; c < FLAT_CHUNKS; c++) if (c < chunks) {
                    const bool here = (reached[c] >> lane) & 1ull;
                    nNodes += here ? 1u : 0u;
                    if constexpr (BRMI_STREAMING_PASS) {
                        if (here && ((seenLeafM[c] >> lane) & 1ull))
                            flat_leaf_touch(BRMI_ST_ARG, a.flatNodes[iw.flatBase + c * 64u + lane], a.flatLeaves[iw.flatBase + c * 64u + lane], instIndex, model, scale, camPos, zNear, threshold, ortho);
                    }
                    const uint64_t rm = a.occlusion ? (reached[c] & hiddenM[c]) : 0ull;
                    replayRank[c] = nReplay + (uint32_t)__popcll(rm & ((1ull << lane) - 1ull));
                    nReplay += (uint32_t)__popcll(rm);
                    const bool emitLeaf = here && ((leafM[c] >> lane) & 1ull);
                    const uint32_t segCount = segFirstCountA[c] >> 16;
                    chunksOfLeaf[c] = emitLeaf ? (segCount + a.factor - 1u) / a.factor : 0u;
                    uint32_t incl = chunksOfLeaf[c];
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, o); if (lane >= (uint32_t)o) incl += v; }
                    bucketRank[c] = nBuckets + incl - chunksOfLeaf[c];
                    nBuckets += (uint32_t)__shfl((int)incl, 63);
                }
                uint32_t replayBase = 0, bucketBase = 0;
                if (lane == 0) {
                    if (nReplay != 0u) replayBase = atomicAdd(&a.counters[CNT_REPLAY_NODES], nReplay);
                    if (nBuckets != 0u) bucketBase = atomicAdd(&a.counters[a.bucketCounter], nBuckets);
                }
                replayBase = (uint32_t)__shfl((int)replayBase, 0); bucketBase = (uint32_t)__shfl((int)bucketBase, 0);
#pragma unroll
                for (uint32_t c = 0; c < FLAT_CHUNKS; c++) if (c < chunks) {
                    if (a.occlusion && ((reached[c] & hiddenM[c]) >> lane) & 1ull) {
                        const uint32_t slot = replayBase + replayRank[c];
                        if (slot < a.recordCapacity) a.replayNodes[slot] = NodeRecord{instIndex, 0x80000000u | (1u << 30) | (nodeIdA[c] & 0x3FFFFFFFu)};
                        else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
                    }
                    // bucket records of `factor` meshlets per reached leaf that passed (computeCulling.hlsl:385-406)
                    const uint32_t segFirst = segFirstCountA[c] & 0xFFFFu, segCount = segFirstCountA[c] >> 16;
                    for (uint32_t k = 0; k < chunksOfLeaf[c]; k++) {
                        const uint32_t slot = bucketBase + bucketRank[c] + k;
                        if (slot >= a.recordCapacity) { atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u); continue; }
                        BucketRecord b;
                        b.instanceIndex = instIndex; b.groupIdPacked = ownerGroupA[c] & 0x7FFFFFFFu;
                        b.meshletIndexAndCount = (min(a.factor, segCount - k * a.factor) << 16) | ((segFirst + k * a.factor) & 0xFFFFu);
                        b.pageSlabDescriptorIndex = slabDescA[c]; b.pageSlabByteOffset = slabOffA[c];
                        b.firstBit = iw.bitBase + firstBitRelA[c] + k * a.factor; b.pad0 = 0; b.pad1 = 0;
                        buckets[slot] = b;
                    }
                }
                continue;
            }
        }
        const uint32_t mdIndex = sc.clodOffsets[instIndex].clodMeshMetadataIndex;
        // this launch handles the meshes whose widest BVH level fits its LDS frontier class, and the top of wider ones
        const uint32_t width = meshLevelWidth[mdIndex];
        if (width < widthLo || width > widthHi) continue;
        const bool spill = width > spillAbove;
        const brmi_clod_mesh_metadata md = sc.meshMetadata[mdIndex];
        const brmi_per_object* obj = sc.perObject + inst.perObjectBufferIndex;
        const m4 model = load_m4(&obj->model[0][0]);
        const float scale = max_axis_scale(model);
        const f3 instC{inst.boundingSphere[0], inst.boundingSphere[1], inst.boundingSphere[2]}; const float instR = inst.boundingSphere[3];
        if (!REPLAY) {
            // K1 (PureComputeObjectCullCS)
            const f3 c = to_view_space(instC, model, view);
            const float r = instR * scale;
            const bool bad = isnan(c.x) || isnan(c.y) || isnan(c.z) || isinf(c.x) || isinf(c.y) || isinf(c.z) || isnan(r) || isinf(r);
            const bool visible = !bad && !sphere_culled(a, cam, c, r);
            nTested++;
            if (!visible) continue;
            nVisible++;
            startNode = md.rootNode;
        }
        const bool skinned = (sc.perMesh[inst.perMeshBufferIndex].vertexFlags & BRMI_VERTEX_SKINNED) != 0;
        const uint32_t bitBase = a.instanceBitBase[instIndex];
        __syncthreads();
        if (lane == 0) { frontier[0][0] = startNode; counts[0] = 1u; counts[1] = 0u; }
        __syncthreads();
        for (uint32_t level = 0; level < 64u; level++) {
            const uint32_t cur = level & 1u, nxt = cur ^ 1u;
            const uint32_t n = min(counts[cur], HIER_CAP);
            if (n == 0u) break;
            if (spill && n > HIER_CAP / BRMI_BVH_MAX_CHILDREN) {      // the level after this one may not fit: the level kernels take over from here
                uint32_t baseSlot = 0;
                if (lane == 0) baseSlot = atomicAdd(&a.counters[CNT_FRONTIER0], n);
                baseSlot = (uint32_t)__shfl((int)baseSlot, 0);
                for (uint32_t k = lane; k < n; k += 64u) {
                    if (baseSlot + k < a.recordCapacity) spillOut[baseSlot + k] = NodeRecord{instIndex, (REPLAY ? 0x80000000u : 0u) | (1u << 30) | (frontier[cur][k] & 0x3FFFFFFFu)};
                    else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
                }
                break;
            }
            for (uint32_t base = 0; base < n; base += 64u) {
                const bool have = base + lane < n;
                bool isInternal = false, emitLeaf = false, occluded = false;
                uint32_t nodeId = 0, childBase = 0, childCount = 0, segFirst = 0, segCount = 0, ownerGroup = 0, slabDesc = 0, slabOff = 0, firstBit = 0;
                if (have) {
                    nodeId = frontier[cur][base + lane];
                    nNodes++;
                    const brmi_lod_node node = sc.lodNodes[md.lodNodesBase + nodeId];
                    const f3 cullC = skinned ? instC : f3{node.cullCenterAndRadius[0], node.cullCenterAndRadius[1], node.cullCenterAndRadius[2]};
                    const float cullR = skinned ? instR : node.cullCenterAndRadius[3];
                    const f3 cVS = to_view_space(cullC, model, view);
                    const float rW = cullR * scale;
                    const bool culled = !REPLAY && sphere_culled(a, cam, cVS, rW);
                    if (!culled) {
                        if (node.isLeaf != BRMI_NODE_INTERNAL) {
                            const brmi_lod_group* g = sc.lodGroups + (md.groupsBase + node.ownerGroupId);
                            const f3 gc = xyz(mul_point(f3{g->centerAndRadius[0], g->centerAndRadius[1], g->centerAndRadius[2]}, model));
                            const float gr = g->centerAndRadius[3] * scale;
                            const float eod = projected_error(gc, gr, node.maxQuadricError, scale, camPos, zNear, ortho);
                            bool ok = eod >= threshold;
                            if constexpr (BRMI_STREAMING_PASS) {
                                if (ok) {
                                    const bool canRender = stream_touch(BRMI_ST_ARG, md.groupsBase + node.ownerGroupId, instIndex, eod);
                                    if (node.countMinusOne != 0u && !(refined_child_eod(sc, md.groupsBase + node.countMinusOne - 1u, model, scale, camPos, zNear, ortho) < threshold) &&
                                        stream_touch(BRMI_ST_ARG, md.groupsBase + node.countMinusOne - 1u, instIndex, eod)) ok = false;
                                    if (!canRender) ok = false;
                                }
                            } else
                            if (ok && refined_child_suppresses(sc, md.groupsBase, node.countMinusOne - 1u, node.countMinusOne != 0u, model, scale, camPos, zNear, threshold, ortho)) ok = false;
                            if (ok) {
                                const brmi_lod_segment seg = sc.lodSegments[md.segmentsBase + node.indexOrOffset];
                                const brmi_group_page_map_entry pe = sc.groupPageMap[md.pageMapBase + seg.pageIndex];
                                if (seg.meshletCount != 0u && pe.slabDescriptorIndex != 0u) {
                                    emitLeaf = true;
                                    segFirst = seg.firstMeshletInPage; segCount = seg.meshletCount; ownerGroup = node.ownerGroupId;
                                    slabDesc = pe.slabDescriptorIndex; slabOff = pe.slabByteOffset;
                                    firstBit = bitBase + a.segPrefix[md.segmentsBase + node.indexOrOffset];
                                }
                            }
                        } else {
                            const f3 lc = xyz(mul_point(f3{node.lodCenterAndRadius[0], node.lodCenterAndRadius[1], node.lodCenterAndRadius[2]}, model));
                            const float lr = node.lodCenterAndRadius[3] * scale;
                            const float nodeEod = projected_error(lc, lr, node.maxQuadricError, scale, camPos, zNear, ortho);
                            if (nodeEod >= threshold) {
                                if (a.occlusion && occlusion_test(a, cam, REPLAY, cullC, cullR, cVS, rW, obj)) occluded = !REPLAY;
                                else { isInternal = true; childBase = node.indexOrOffset; childCount = min(node.countMinusOne + 1u, BRMI_BVH_MAX_CHILDREN); }
                            }
                        }
                    }
                }
                if (!REPLAY && a.occlusion) {
                    const uint32_t slot = wave_append(&a.counters[CNT_REPLAY_NODES], occluded);
                    if (occluded) {
                        if (slot < a.recordCapacity) a.replayNodes[slot] = NodeRecord{instIndex, 0x80000000u | (1u << 30) | (nodeId & 0x3FFFFFFFu)};
                        else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
                    }
                }
                {   // leaf: bucket records of `factor` meshlets (computeCulling.hlsl:385-406).  One reservation for the whole wave
                    // (an atomic with return per chunk would put ~2 us of latency on every chunk of this single-wave workgroup).
                    const uint32_t nChunks = emitLeaf ? (segCount + a.factor - 1u) / a.factor : 0u;
                    uint32_t incl = nChunks;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, o); if (lane >= (uint32_t)o) incl += v; }
                    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
                    if (total != 0u) {
                        if (staged + total > HIER_STAGE) flush();
                        if (total <= HIER_STAGE) {
                            const uint32_t baseSlot = staged + (incl - nChunks);
                            for (uint32_t k = 0; k < nChunks; k++) {
                                const uint32_t first = segFirst + k * a.factor;
                                const uint32_t cnt = min(a.factor, segCount - k * a.factor);
                                BucketRecord b;
                                b.instanceIndex = instIndex; b.groupIdPacked = (REPLAY ? 0x80000000u : 0u) | (ownerGroup & 0x7FFFFFFFu);
                                b.meshletIndexAndCount = (cnt << 16) | (first & 0xFFFFu);
                                b.pageSlabDescriptorIndex = slabDesc; b.pageSlabByteOffset = slabOff;
                                b.firstBit = firstBit + k * a.factor; b.pad0 = 0; b.pad1 = 0;
                                stage[baseSlot + k] = b;
                            }
                            staged += total;
                        } else {
                            // more chunks in one step than the stage holds (very large segments): straight to the global array
                            uint32_t baseSlot = 0;
                            if (lane == 0) baseSlot = atomicAdd(&a.counters[a.bucketCounter], total);
                            baseSlot = (uint32_t)__shfl((int)baseSlot, 0) + (incl - nChunks);
                            for (uint32_t k = 0; k < nChunks; k++) {
                                const uint32_t slot = baseSlot + k;
                                if (slot < a.recordCapacity) {
                                    const uint32_t first = segFirst + k * a.factor;
                                    const uint32_t cnt = min(a.factor, segCount - k * a.factor);
                                    BucketRecord b;
                                    b.instanceIndex = instIndex; b.groupIdPacked = (REPLAY ? 0x80000000u : 0u) | (ownerGroup & 0x7FFFFFFFu);
                                    b.meshletIndexAndCount = (cnt << 16) | (first & 0xFFFFu);
                                    b.pageSlabDescriptorIndex = slabDesc; b.pageSlabByteOffset = slabOff;
                                    b.firstBit = firstBit + k * a.factor; b.pad0 = 0; b.pad1 = 0;
                                    buckets[slot] = b;
                                } else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
                            }
                        }
                    }
                }
                {   // internal: pre-filter the children, survivors go to the next level's frontier (computeCulling.hlsl:477-530).
                    // The children of all nodes of this step are dealt to the lanes (exclusive scan of the child counts), so their
                    // node records are fetched side by side instead of one dependent round trip per child index.
                    const uint32_t myChildren = isInternal ? childCount : 0u;
                    uint32_t incl = myChildren;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, o); if (lane >= (uint32_t)o) incl += v; }
                    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
                    if (total != 0u) {
                        childOff[lane] = incl - myChildren; childFirst[lane] = childBase;
                        if (lane == 63) childOff[64] = total;
                        __syncthreads();
                        for (uint32_t task = lane; task < ((total + 63u) & ~63u); task += 64u) {
                            bool emit = false;
                            uint32_t childId = 0;
                            if (task < total) {
                                uint32_t parent = 0;
#pragma unroll
                                for (uint32_t step = 32; step > 0; step >>= 1) if (childOff[parent + step] <= task) parent += step;
                                childId = childFirst[parent] + (task - childOff[parent]);
                                const brmi_lod_node* ch = sc.lodNodes + (md.lodNodesBase + childId);
                                const f3 cc = skinned ? instC : f3{ch->cullCenterAndRadius[0], ch->cullCenterAndRadius[1], ch->cullCenterAndRadius[2]};
                                const float cr = skinned ? instR : ch->cullCenterAndRadius[3];
                                const f3 ccVS = to_view_space(cc, model, view);
                                emit = REPLAY || !sphere_culled(a, cam, ccVS, cr * scale);
                                if (emit && ch->isLeaf == BRMI_NODE_INTERNAL) {
                                    const f3 wc = xyz(mul_point(f3{ch->lodCenterAndRadius[0], ch->lodCenterAndRadius[1], ch->lodCenterAndRadius[2]}, model));
                                    const float e = projected_error(wc, ch->lodCenterAndRadius[3] * scale, ch->maxQuadricError, scale, camPos, zNear, ortho);
                                    if (e < threshold) emit = false;
                                }
                            }
                            const uint32_t slot = wave_append(&counts[nxt], emit);
                            if (emit) {
                                if (slot < HIER_CAP) frontier[nxt][slot] = childId;
                                else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
                            }
                        }
                        __syncthreads();
                    }
                }
            }
            __syncthreads();
            if (lane == 0) counts[cur] = 0u;
            __syncthreads();
        }
    }
    flush();
    // statistics: one atomic per wave and counter, on one of 64 stripes (every stripe has its own 128 B line: thousands of
    // same-line atomics serialise at ~90 per microsecond); brmi_read_counters adds the stripes up
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nNodes += (uint32_t)__shfl_xor((int)nNodes, o);
    if (lane == 0) {
        uint32_t* stripe = a.counters + CNT_STRIPES + (blockIdx.x & (CNT_STRIPE_COUNT - 1u)) * CNT_STRIPE_WORDS;
        if (nTested) atomicAdd(&stripe[0], nTested);
        if (nVisible) atomicAdd(&stripe[1], nVisible);
        if (nNodes) atomicAdd(&stripe[2], nNodes);
    }
}

// Flat evaluation of a hierarchy of 257 .. 8192 nodes (the dense workload's terrain-like meshes: 4,270 nodes, six levels): one 1024-thread
// workgroup per draw, a node per thread and chunk of 1024, the per-node verdicts and parent links in LDS, "reached" propagated there, one pair of
// reservations per draw.  The level walk spent a launch per level on such a mesh (k_traverse: ~10 us each, three per phase) behind a chain of
// LDS-walk steps; here every node of the hierarchy is fetched in at most eight rounds whatever the depth.  Same tests, same records.
__global__ void __launch_bounds__(1024) BRMI_CULL_KERNEL(k_cull_flat_wide)(CullArgs a, BucketRecord* buckets BRMI_ST_PARAM) {
    __shared__ uint8_t verdict[FLAT_WIDE_MAX];          // bit 0 passes as a child, 1 lets its children through, 2 hidden by the depth chain, 3 leaf that emits, 4 reached
    __shared__ uint16_t parentOf[FLAT_WIDE_MAX], recordsOf[FLAT_WIDE_MAX];
    __shared__ uint32_t waveSum[2][16], changed, bases[2];
    const brmi_scene_buffers& sc = a.sc;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t viewId = sc.perFrame->mainCameraIndex;
    const brmi_camera* cam = sc.cameras + viewId;
    const brmi_culling_camera* lodCam = sc.cullingCameras + viewId;
    const bool ortho = cam->isOrtho != 0;
    const f3 camPos{lodCam->positionWorldSpace[0], lodCam->positionWorldSpace[1], lodCam->positionWorldSpace[2]};
    const float zNear = lodCam->zNear, threshold = lodCam->errorOverDistanceThreshold;
    const m4 view = load_m4(&cam->view[0][0]);
    uint32_t nTested = 0, nVisible = 0, nNodes = 0;
    for (uint32_t seed = blockIdx.x; seed < sc.activeDrawCount; seed += gridDim.x) {
        const uint32_t instIndex = sc.activeDraws[seed];
        const InstanceWalk iw = a.instanceWalk[instIndex];
        if (iw.flatCount <= 256u || iw.flatCount > FLAT_WIDE_MAX) continue;          // (block-uniform) the walk's, or not flat at all
        const brmi_per_mesh_instance inst = sc.perMeshInstance[instIndex];
        const brmi_per_object* obj = sc.perObject + inst.perObjectBufferIndex;
        const m4 model = load_m4(&obj->model[0][0]);
        const m4 prevModel = a.occlusion ? load_m4(&obj->prevModel[0][0]) : model;
        const float scale = max_axis_scale(model);
        const f3 instC{inst.boundingSphere[0], inst.boundingSphere[1], inst.boundingSphere[2]}; const float instR = inst.boundingSphere[3];
        {   // K1 (PureComputeObjectCullCS)
            const f3 c = to_view_space(instC, model, view);
            const float r = instR * scale;
            const bool bad = isnan(c.x) || isnan(c.y) || isnan(c.z) || isinf(c.x) || isinf(c.y) || isinf(c.z) || isnan(r) || isinf(r);
            if (t == 0) nTested++;
            if (bad || sphere_culled(a, cam, c, r)) continue;
            if (t == 0) nVisible++;
        }
        const bool skinned = iw.skinned != 0u;
        __syncthreads();                                    // the previous draw's LDS state has been read
        for (uint32_t node = t; node < iw.flatCount; node += 1024u) {
            const FlatNode fn = a.flatNodes[iw.flatBase + node];
            const bool internal = (fn.info & 1u);
            const f3 cullC = skinned ? instC : f3{fn.cull[0], fn.cull[1], fn.cull[2]};
            const float cullR = skinned ? instR : fn.cull[3];
            const f3 cVS = to_view_space(cullC, model, view);
            const float rW = cullR * scale;
            const bool inFrustum = !sphere_culled(a, cam, cVS, rW);
            bool pre = inFrustum, expand = false, hidden = false, leafOk = false;
            uint32_t records = 0;
            if (inFrustum && internal) {
                const f3 lc = xyz(mul_point(f3{fn.lod[0], fn.lod[1], fn.lod[2]}, model));
                const float e = projected_error(lc, fn.lod[3] * scale, fn.maxQuadricError, scale, camPos, zNear, ortho);
                pre = e >= threshold;
                if (pre) { hidden = a.occlusion && occlusion_test_prev(a, cam, cullC, cullR, prevModel); expand = !hidden; }
            } else if (inFrustum) {
                const FlatLeaf fl = a.flatLeaves[iw.flatBase + node];
                const f3 gc = xyz(mul_point(f3{fl.group[0], fl.group[1], fl.group[2]}, model));
                const float eod = projected_error(gc, fl.group[3] * scale, fn.maxQuadricError, scale, camPos, zNear, ortho);
                bool ok = eod >= threshold;
                if (ok && ((fn.info >> 1) & 1u)) {      // refined_child_suppresses
                    const f3 cc = xyz(mul_point(f3{fl.child[0], fl.child[1], fl.child[2]}, model));
                    const float ce = projected_error(cc, fl.child[3] * scale, fl.childParentError, scale, camPos, zNear, ortho);
                    if (!(ce < threshold)) {
                        if constexpr (BRMI_STREAMING_PASS) { if (stream_resident(BRMI_ST_ARG, fl.childGlobal)) ok = false; } else ok = false;
                    }
                }
                if constexpr (BRMI_STREAMING_PASS) { if (ok && !stream_resident(BRMI_ST_ARG, fl.ownerGlobal)) ok = false; }
                if (ok && ((fn.info >> 2) & 1u)) {
                    leafOk = sc.groupPageMap[fn.pageMapIndex].slabDescriptorIndex != 0u;
                    records = leafOk ? ((fn.segFirstCount >> 16) + a.factor - 1u) / a.factor : 0u;
                }
            }
            if constexpr (BRMI_STREAMING_PASS) verdict[node] = (uint8_t)((pre ? 1u : 0u) | (expand ? 2u : 0u) | (hidden ? 4u : 0u) | (leafOk ? 8u : 0u) | (node == 0u ? 16u : 0u) | ((inFrustum && !internal) ? 32u : 0u));      // (bit 5: a leaf that reached its error test)
            else
            verdict[node] = (uint8_t)((pre ? 1u : 0u) | (expand ? 2u : 0u) | (hidden ? 4u : 0u) | (leafOk ? 8u : 0u) | (node == 0u ? 16u : 0u));
            parentOf[node] = (uint16_t)(fn.info >> 8); recordsOf[node] = (uint16_t)records;
        }
        // reached: the root, or a node that passed as a child of a reached node that lets its children through (parents lie below their
        // children in the breadth-first order, so a sweep settles a level at least)
        for (;;) {
            __syncthreads();
            if (t == 0) changed = 0u;
            __syncthreads();
            for (uint32_t node = t; node < iw.flatCount; node += 1024u) {
                const uint32_t v = verdict[node];
                if (!(v & 16u) && (v & 1u)) { const uint32_t pv = verdict[parentOf[node]]; if ((pv & 18u) == 18u) { verdict[node] = (uint8_t)(v | 16u); changed = 1u; } }
            }
            __syncthreads();
            if (changed == 0u) break;
        }
        // per thread: its nodes' replay records and bucket records, then a block-wide exclusive scan of both
        uint32_t myReplay = 0, myBuckets = 0;
        for (uint32_t node = t; node < iw.flatCount; node += 1024u) {
            const uint32_t v = verdict[node];
            if (v & 16u) { nNodes++; if (a.occlusion && (v & 4u)) myReplay++; if (v & 8u) myBuckets += recordsOf[node]; }
        }
        uint32_t inclR = myReplay, inclB = myBuckets;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t r = (uint32_t)__shfl_up((int)inclR, o), b = (uint32_t)__shfl_up((int)inclB, o); if (lane >= (uint32_t)o) { inclR += r; inclB += b; } }
        if (lane == 63u) { waveSum[0][wave] = inclR; waveSum[1][wave] = inclB; }
        __syncthreads();
        uint32_t baseR = 0, baseB = 0, totalR = 0, totalB = 0;
        for (uint32_t w = 0; w < 16u; w++) { if (w < wave) { baseR += waveSum[0][w]; baseB += waveSum[1][w]; } totalR += waveSum[0][w]; totalB += waveSum[1][w]; }
        if (t == 0) {
            bases[0] = totalR ? atomicAdd(&a.counters[CNT_REPLAY_NODES], totalR) : 0u;
            bases[1] = totalB ? atomicAdd(&a.counters[a.bucketCounter], totalB) : 0u;
        }
        __syncthreads();
        uint32_t slotR = bases[0] + baseR + inclR - myReplay, slotB = bases[1] + baseB + inclB - myBuckets;
        for (uint32_t node = t; node < iw.flatCount; node += 1024u) {
            const uint32_t v = verdict[node];
            if (!(v & 16u)) continue;
            if constexpr (BRMI_STREAMING_PASS) { if (v & 32u) flat_leaf_touch(BRMI_ST_ARG, a.flatNodes[iw.flatBase + node], a.flatLeaves[iw.flatBase + node], instIndex, model, scale, camPos, zNear, threshold, ortho); }
            if (a.occlusion && (v & 4u)) {
                const FlatNode fn = a.flatNodes[iw.flatBase + node];
                if (slotR < a.recordCapacity) a.replayNodes[slotR] = NodeRecord{instIndex, 0x80000000u | (1u << 30) | (fn.nodeId & 0x3FFFFFFFu)};
                else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
                slotR++;
            }
            if (v & 8u) {
                const FlatNode fn = a.flatNodes[iw.flatBase + node];
                const brmi_group_page_map_entry pe = sc.groupPageMap[fn.pageMapIndex];
                const uint32_t segFirst = fn.segFirstCount & 0xFFFFu, segCount = fn.segFirstCount >> 16;
                for (uint32_t k = 0; k < recordsOf[node]; k++, slotB++) {
                    if (slotB >= a.recordCapacity) { atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u); continue; }
                    BucketRecord b;
                    b.instanceIndex = instIndex; b.groupIdPacked = fn.ownerGroup & 0x7FFFFFFFu;
                    b.meshletIndexAndCount = (min(a.factor, segCount - k * a.factor) << 16) | ((segFirst + k * a.factor) & 0xFFFFu);
                    b.pageSlabDescriptorIndex = pe.slabDescriptorIndex; b.pageSlabByteOffset = pe.slabByteOffset;
                    b.firstBit = iw.bitBase + fn.firstBitRel + k * a.factor; b.pad0 = 0; b.pad1 = 0;
                    buckets[slotB] = b;
                }
            }
        }
    }
    // statistics: one atomic per wave and counter on a stripe of its own
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nNodes += (uint32_t)__shfl_xor((int)nNodes, o);
    if (lane == 0) {
        uint32_t* stripe = a.counters + CNT_STRIPES + ((blockIdx.x * 16u + wave) & (CNT_STRIPE_COUNT - 1u)) * CNT_STRIPE_WORDS;
        if (nTested) atomicAdd(&stripe[0], nTested);
        if (nVisible) atomicAdd(&stripe[1], nVisible);
        if (nNodes) atomicAdd(&stripe[2], nNodes);
    }
}

// Level-synchronous flat traversal for scenes of MANY draws (Zorah-class: 100 k instances of two 600-node hierarchies, 83 k of them in the frustum,
// seven nodes reached in each on average).  One wave per draw -- the LDS walk above, or the flat evaluation of every node -- keeps the chip busy with
// chains of dependent loads: 83 k instances x ~25 us of chain over the ~3 k waves that fit is 0.7 ms (measured 0.7 - 1.0 ms, and its one
// reservation per draw on one counter, served at ~90 per microsecond, costs as much again), and evaluating all 600 nodes of every instance is 3 ms.
// Here a LANE is a task: level 0 takes a draw (K1, then the root), every later level a (instance, flat position) record of the frontier the level
// before wrote; a node's children sit side by side in the breadth-first tables (FlatNode::children), so their pre-filter is eight independent
// loads.  Appends are aggregated per workgroup (three atomics per 256 tasks).  Same tests, same arithmetic, same records as the walk; the order of
// the bucket records differs, which the survivor ranking (a bit per (instance, segment, meshlet)) does not see.  flatMaxDepth launches.
template <bool FIRST>
__global__ void __launch_bounds__(256) BRMI_CULL_KERNEL(k_cull_flat_level)(CullArgs a, uint32_t level, const NodeRecord* in, NodeRecord* out, BucketRecord* buckets BRMI_ST_PARAM) {
    __shared__ uint32_t waveTot[3][4], bases[3];
    const brmi_scene_buffers& sc = a.sc;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t viewId = sc.perFrame->mainCameraIndex;
    const brmi_camera* cam = sc.cameras + viewId;
    const brmi_culling_camera* lodCam = sc.cullingCameras + viewId;
    const bool ortho = cam->isOrtho != 0;
    const f3 camPos{lodCam->positionWorldSpace[0], lodCam->positionWorldSpace[1], lodCam->positionWorldSpace[2]};
    const float zNear = lodCam->zNear, threshold = lodCam->errorOverDistanceThreshold;
    const m4 view = load_m4(&cam->view[0][0]);
    const uint32_t count = FIRST ? sc.activeDrawCount : min(a.counters[CNT_FRONTIER0 + level], a.recordCapacity);
    uint32_t* nextCount = &a.counters[CNT_FRONTIER0 + level + 1u];
    const uint32_t rounded = (count + 255u) & ~255u;        // workgroup-uniform trip count (barriers inside)
    uint32_t nTested = 0, nVisible = 0, nNodes = 0;
    for (uint32_t idx = blockIdx.x * 256u + t; idx < rounded; idx += gridDim.x * 256u) {
        bool have = idx < count;
        uint32_t instIndex = 0, pos = 0;
        InstanceWalk iw{0u, 0u, 0u, 0u}; brmi_per_mesh_instance inst{};
        if (have) {
            if (FIRST) instIndex = sc.activeDraws[idx];
            else { const NodeRecord rec = in[idx]; instIndex = rec.instanceIndex; pos = rec.nodeIdPacked; }
            iw = a.instanceWalk[instIndex]; inst = sc.perMeshInstance[instIndex];
            if (iw.flatCount == 0u) have = false;         // (launch_cull takes this path only when every mesh has flat tables)
        }
        bool hidden = false, leafOk = false;
        uint32_t childMask = 0, firstChild = 0, nChunks = 0, slabDesc = 0, slabOff = 0;
        FlatNode fn{};
        if (have) {
            const brmi_per_object* obj = sc.perObject + inst.perObjectBufferIndex;
            const m4 model = load_m4(&obj->model[0][0]);
            const float scale = max_axis_scale(model);
            const f3 instC{inst.boundingSphere[0], inst.boundingSphere[1], inst.boundingSphere[2]}; const float instR = inst.boundingSphere[3];
            if (FIRST) {   // K1 (PureComputeObjectCullCS)
                const f3 c = to_view_space(instC, model, view);
                const float r = instR * scale;
                const bool bad = isnan(c.x) || isnan(c.y) || isnan(c.z) || isinf(c.x) || isinf(c.y) || isinf(c.z) || isnan(r) || isinf(r);
                nTested++;
                if (bad || sphere_culled(a, cam, c, r)) have = false; else nVisible++;
            }
            if (have) {
                nNodes++;
                fn = a.flatNodes[iw.flatBase + pos];
                const bool skinned = iw.skinned != 0u;
                const bool internal = (fn.info & 1u);
                const f3 cullC = skinned ? instC : f3{fn.cull[0], fn.cull[1], fn.cull[2]};
                const float cullR = skinned ? instR : fn.cull[3];
                const f3 cVS = to_view_space(cullC, model, view);
                const float rW = cullR * scale;
                const bool inFrustum = !sphere_culled(a, cam, cVS, rW);
                if (inFrustum && internal) {
                    const f3 lc = xyz(mul_point(f3{fn.lod[0], fn.lod[1], fn.lod[2]}, model));
                    const float e = projected_error(lc, fn.lod[3] * scale, fn.maxQuadricError, scale, camPos, zNear, ortho);
                    if (e >= threshold) {
                        hidden = a.occlusion && occlusion_test_prev(a, cam, cullC, cullR, load_m4(&obj->prevModel[0][0]));
                        if (!hidden) {
                            // the children that pass as children: in the frustum and, internal ones, above the error threshold (computeCulling.hlsl:477-530)
                            firstChild = fn.children & 0xFFFFu;
                            const uint32_t cc = min(fn.children >> 16, BRMI_BVH_MAX_CHILDREN);
#pragma unroll
                            for (uint32_t c = 0; c < BRMI_BVH_MAX_CHILDREN; c++) if (c < cc) {
                                const FlatNode* ch = a.flatNodes + (iw.flatBase + firstChild + c);
                                const float4 cs = *reinterpret_cast<const float4*>(ch->cull), ls = *reinterpret_cast<const float4*>(ch->lod);
                                const float chErr = ch->maxQuadricError; const uint32_t chInfo = ch->info;
                                const f3 ccVS = to_view_space(skinned ? instC : f3{cs.x, cs.y, cs.z}, model, view);
                                bool pre = !sphere_culled(a, cam, ccVS, (skinned ? instR : cs.w) * scale);
                                if (pre && (chInfo & 1u)) {
                                    const f3 wc = xyz(mul_point(f3{ls.x, ls.y, ls.z}, model));
                                    pre = projected_error(wc, ls.w * scale, chErr, scale, camPos, zNear, ortho) >= threshold;
                                }
                                childMask |= pre ? (1u << c) : 0u;
                            }
                        }
                    }
                } else if (inFrustum) {
                    const FlatLeaf fl = a.flatLeaves[iw.flatBase + pos];
                    if constexpr (BRMI_STREAMING_PASS) flat_leaf_touch(BRMI_ST_ARG, fn, fl, instIndex, model, scale, camPos, zNear, threshold, ortho);      // (a task IS a reached node)
                    const f3 gc = xyz(mul_point(f3{fl.group[0], fl.group[1], fl.group[2]}, model));
                    const float eod = projected_error(gc, fl.group[3] * scale, fn.maxQuadricError, scale, camPos, zNear, ortho);
                    bool ok = eod >= threshold;
                    if (ok && ((fn.info >> 1) & 1u)) {      // refined_child_suppresses
                        const f3 cc = xyz(mul_point(f3{fl.child[0], fl.child[1], fl.child[2]}, model));
                        const float ce = projected_error(cc, fl.child[3] * scale, fl.childParentError, scale, camPos, zNear, ortho);
                        if (!(ce < threshold)) {
                            if constexpr (BRMI_STREAMING_PASS) { if (stream_resident(BRMI_ST_ARG, fl.childGlobal)) ok = false; } else ok = false;
                        }
                    }
                    if constexpr (BRMI_STREAMING_PASS) { if (ok && !stream_resident(BRMI_ST_ARG, fl.ownerGlobal)) ok = false; }
                    if (ok && ((fn.info >> 2) & 1u)) {
                        const brmi_group_page_map_entry pe = sc.groupPageMap[fn.pageMapIndex];
                        slabDesc = pe.slabDescriptorIndex; slabOff = pe.slabByteOffset;
                        leafOk = slabDesc != 0u;
                        nChunks = leafOk ? ((fn.segFirstCount >> 16) + a.factor - 1u) / a.factor : 0u;
                    }
                }
            }
        }
        // one reservation per workgroup and output: frontier records, bucket records, replay nodes
        const uint32_t mine[3] = {(uint32_t)__popc(childMask), nChunks, hidden ? 1u : 0u};
        uint32_t incl[3] = {mine[0], mine[1], mine[2]};
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
            for (int q = 0; q < 3; q++) { const uint32_t v = (uint32_t)__shfl_up((int)incl[q], o); if (lane >= (uint32_t)o) incl[q] += v; }
        }
        __syncthreads();                                 // the previous round's bases have been read
        if (lane == 63u) { waveTot[0][wave] = incl[0]; waveTot[1][wave] = incl[1]; waveTot[2][wave] = incl[2]; }
        __syncthreads();
        if (t < 3u) {
            const uint32_t total = waveTot[t][0] + waveTot[t][1] + waveTot[t][2] + waveTot[t][3];
            uint32_t* counter = t == 0u ? nextCount : (t == 1u ? &a.counters[a.bucketCounter] : &a.counters[CNT_REPLAY_NODES]);
            bases[t] = total ? atomicAdd(counter, total) : 0u;
        }
        __syncthreads();
        uint32_t slot[3];
#pragma unroll
        for (int q = 0; q < 3; q++) { uint32_t wb = 0; for (uint32_t w = 0; w < 4u; w++) if (w < wave) wb += waveTot[q][w]; slot[q] = bases[q] + wb + incl[q] - mine[q]; }
        for (uint32_t m = childMask; m != 0u; m &= m - 1u, slot[0]++) {
            if (slot[0] < a.recordCapacity) out[slot[0]] = NodeRecord{instIndex, firstChild + (uint32_t)__ffs((int)m) - 1u};
            else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
        }
        if (nChunks != 0u) {
            const uint32_t segFirst = fn.segFirstCount & 0xFFFFu, segCount = fn.segFirstCount >> 16;
            for (uint32_t k = 0; k < nChunks; k++, slot[1]++) {
                if (slot[1] >= a.recordCapacity) { atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u); continue; }
                BucketRecord b;
                b.instanceIndex = instIndex; b.groupIdPacked = fn.ownerGroup & 0x7FFFFFFFu;
                b.meshletIndexAndCount = (min(a.factor, segCount - k * a.factor) << 16) | ((segFirst + k * a.factor) & 0xFFFFu);
                b.pageSlabDescriptorIndex = slabDesc; b.pageSlabByteOffset = slabOff;
                b.firstBit = iw.bitBase + fn.firstBitRel + k * a.factor; b.pad0 = 0; b.pad1 = 0;
                buckets[slot[1]] = b;
            }
        }
        if (hidden) {
            if (slot[2] < a.recordCapacity) a.replayNodes[slot[2]] = NodeRecord{instIndex, 0x80000000u | (1u << 30) | (fn.nodeId & 0x3FFFFFFFu)};
            else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
        }
    }
    // statistics: one atomic per wave and counter on a stripe of its own
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nNodes += (uint32_t)__shfl_xor((int)nNodes, o); nTested += (uint32_t)__shfl_xor((int)nTested, o); nVisible += (uint32_t)__shfl_xor((int)nVisible, o); }
    if (lane == 0) {
        uint32_t* stripe = a.counters + CNT_STRIPES + ((blockIdx.x * 4u + wave) & (CNT_STRIPE_COUNT - 1u)) * CNT_STRIPE_WORDS;
        if (nTested) atomicAdd(&stripe[0], nTested);
        if (nVisible) atomicAdd(&stripe[1], nVisible);
        if (nNodes) atomicAdd(&stripe[2], nNodes);
    }
}

// K3: per-meshlet cull ---------------------------------------------------------------------------
// SIDE: workgroups behind the first `mainBlocks` run the second half of the light clustering (page prefix + fill; four clusters each)
// SIDE == 2 (split frames, round 4): the workgroups behind the first `mainBlocks` clear the visibility keys instead.  As riders of the traversal's
// launch the clear's 8,192 and the light clustering's 3,456 single-wave workgroups inherit the walk's 150 VGPRs; beside another frame's shading waves
// (3 x 136 of a SIMD's 512 registers taken) each of them waited for a shading wave to retire -- k_cull_hierarchy 38 us alone, 97 us in flight
// (kernel trace), on the chain the next frame waits for.  This kernel's waves fit the gap (<= 104 registers), and the light clustering of a split
// frame runs on the shading stream (brmi_execute_split).
template <int SIDE>
__global__ void __launch_bounds__(256) BRMI_CULL_KERNEL(k_cull_clusters)(CullArgs a, const BucketRecord* buckets, TempVisible* temp, uint32_t* bitmask, uint8_t* blockDirty,
                                                       typename std::conditional<SIDE == 1, LcRide, typename std::conditional<SIDE == 2, ClearRide, NoSide>::type>::type ride BRMI_ST_PARAM) {
    uint32_t mainBlocks = gridDim.x;
    if constexpr (SIDE == 1) {
        mainBlocks = ride.mainBlocks;
        if (blockIdx.x >= ride.mainBlocks) { lc_fill_block(ride.lc, blockIdx.x - ride.mainBlocks, threadIdx.x); return; }
    }
    if constexpr (SIDE == 2) {
        mainBlocks = ride.mainBlocks;
        if (blockIdx.x >= ride.mainBlocks) {
            const uint64_t stride = (uint64_t)ride.clearBlocks * 256u;
            for (uint64_t i = (uint64_t)(blockIdx.x - ride.mainBlocks) * 256u + threadIdx.x; i < ride.n2; i += stride) ride.vis2[i] = make_ulonglong2(BRMI_VIS_EMPTY, BRMI_VIS_EMPTY);
            return;
        }
    }
    const brmi_scene_buffers& sc = a.sc;
    const uint32_t bucketCount = min(a.counters[a.bucketCounter], a.recordCapacity);
    if (a.feedback && blockIdx.x == 0u && threadIdx.x == 0u) __hip_atomic_store(a.feedback + (a.phase == 1u ? 2 : 4), bucketCount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const uint32_t viewId = sc.perFrame->mainCameraIndex;
    const brmi_camera* cam = sc.cameras + viewId;
    const brmi_culling_camera* lodCam = sc.cullingCameras + viewId;
    const bool ortho = cam->isOrtho != 0;
    const f3 camPos{lodCam->positionWorldSpace[0], lodCam->positionWorldSpace[1], lodCam->positionWorldSpace[2]};
    const float zNear = lodCam->zNear, threshold = lodCam->errorOverDistanceThreshold;
    const m4 view = load_m4(&cam->view[0][0]);
    uint32_t* tempCount = &a.counters[a.phase == 2 ? CNT_TEMP_VISIBLE2 : CNT_TEMP_VISIBLE];
    // one lane per (bucket, meshlet-in-bucket): `factor` lanes cooperate on a record
    const uint64_t totalLanes = (uint64_t)bucketCount * a.factor;
    const uint64_t rounded = (totalLanes + 255ull) & ~255ull;      // workgroup-uniform trip count (barriers inside)
    // (round 5: the survivors' and the occluded meshlets' slots are reserved once per workgroup -- a Zorah-class frame tests 850 k meshlets, and one
    // atomic with return per wave and list, 11 k on two lines, was a third of the kernel)
    __shared__ uint32_t waveSurv[4], waveOccl[4], blockSlots[2];
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < rounded; idx += (uint64_t)mainBlocks * blockDim.x) {
        bool survives = false, occluded = false, tested = false;
        uint4 packed = make_uint4(0, 0, 0, 0);
        uint32_t bit = 0;
        uint4 againLo = make_uint4(0u, 0u, 0u, 0u); uint2 againHi = make_uint2(0u, 0u);      // the replay record of an occluded meshlet (as plain words: a BucketRecord object here left an unused 36 B stack slot in the kernel's descriptor)
        if (idx < totalLanes) {
            const uint32_t bi = (uint32_t)(idx / a.factor), m = (uint32_t)(idx % a.factor);
            const BucketRecord b = buckets[bi];
            const uint32_t count = b.meshletIndexAndCount >> 16, first = b.meshletIndexAndCount & 0xFFFFu;
            if (m < count && b.pageSlabDescriptorIndex != 0u) {
                tested = true;
                const bool replay = (b.groupIdPacked >> 31) != 0;
                const uint32_t lm = first + m;
                const uint8_t* slab = sc.slabs[b.pageSlabDescriptorIndex];
                const brmi_page_header* hdr = reinterpret_cast<const brmi_page_header*>(slab + b.pageSlabByteOffset);
                if (lm < hdr->meshletCount) {
                    const brmi_meshlet_descriptor* desc = reinterpret_cast<const brmi_meshlet_descriptor*>(slab + b.pageSlabByteOffset + hdr->descriptorOffset + lm * 64u);
                    float4 bounds = *reinterpret_cast<const float4*>(desc->bounds);
                    const uint32_t triAndRefined = desc->triangleCountAndRefinedGroup;
                    const brmi_per_mesh_instance inst = sc.perMeshInstance[b.instanceIndex];
                    if ((sc.perMesh[inst.perMeshBufferIndex].vertexFlags & BRMI_VERTEX_SKINNED) != 0u)
                        bounds = skinned_meshlet_bounds(sc, desc, hdr, slab + b.pageSlabByteOffset, inst.skinningInstanceSlot, bounds);
                    const brmi_clod_mesh_metadata* md = sc.meshMetadata + sc.clodOffsets[b.instanceIndex].clodMeshMetadataIndex;
                    const m4 model = load_m4(&sc.perObject[inst.perObjectBufferIndex].model[0][0]);
                    const float scale = max_axis_scale(model);
                    const f3 cVS = to_view_space(f3{bounds.x, bounds.y, bounds.z}, model, view);
                    const float rW = bounds.w * scale;
                    survives = replay || !sphere_outside_frustum(cVS, rW, cam->clippingPlanes);
                    if (survives) {
                        const int refined = (int)(triAndRefined >> 16) - 1;
                        if constexpr (BRMI_STREAMING_PASS) {
                            // condition 2 under the residency rule: a refined child that is not there does not suppress; it is touched and asked for with the
                            // priority of the meshlet's OWN group (its error over distance from bounds.error, workGraphCulling.hlsl:2550-2561)
                            if (refined >= 0 && !(refined_child_eod(sc, md->groupsBase + (uint32_t)refined, model, scale, camPos, zNear, ortho) < threshold)) {
                                const brmi_lod_group* own = sc.lodGroups + (md->groupsBase + (b.groupIdPacked & 0x7FFFFFFFu));
                                const f3 oc = xyz(mul_point(f3{own->centerAndRadius[0], own->centerAndRadius[1], own->centerAndRadius[2]}, model));
                                const float ownEod = projected_error(oc, own->centerAndRadius[3] * scale, own->error, scale, camPos, zNear, ortho);
                                if (stream_touch(BRMI_ST_ARG, md->groupsBase + (uint32_t)refined, b.instanceIndex, ownEod)) survives = false;
                            }
                        } else
                        if (refined_child_suppresses(sc, md->groupsBase, (uint32_t)refined, refined >= 0, model, scale, camPos, zNear, threshold, ortho)) survives = false;
                    }
                    if (survives && a.bandActive) {
                        // tile-bounds test of the screen-tile split: conservative sphere vs the band's two planes
                        if (dot3(f3{a.bandTop[0], a.bandTop[1], a.bandTop[2]}, cVS) < -rW || dot3(f3{a.bandBottom[0], a.bandBottom[1], a.bandBottom[2]}, cVS) < -rW) survives = false;
                    }
                    if (survives && stripe_on(a.stripes) && stripe_rejects(a.stripes, cam, cVS, rW)) survives = false;      // no row of this GPU's: dropped, not replayed
                    if (survives && a.occlusion &&
                        occlusion_test(a, cam, replay, f3{bounds.x, bounds.y, bounds.z}, bounds.w, cVS, rW, sc.perObject + inst.perObjectBufferIndex)) {
                        survives = false;
                        if (!replay) {
                            occluded = true;
                            againLo = make_uint4(b.instanceIndex, 0x80000000u | (b.groupIdPacked & 0x7FFFFFFFu), (1u << 16) | (lm & 0xFFFFu), b.pageSlabDescriptorIndex);
                            againHi = make_uint2(b.pageSlabByteOffset, b.firstBit + m);
                        }
                    }
                    if (survives) {
                        packed = pack_visible_cluster(viewId, b.instanceIndex, lm, b.groupIdPacked & 0x7FFFFFFFu, b.pageSlabDescriptorIndex, b.pageSlabByteOffset);
                        bit = b.firstBit + m;
                    }
                }
            }
        }
        {   // statistics: one atomic per wave on one of 64 stripes
            const uint64_t tm = __ballot(tested);
            if (tm != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(&a.counters[CNT_STRIPES + (blockIdx.x & (CNT_STRIPE_COUNT - 1u)) * CNT_STRIPE_WORDS + STRIPE_MESHLETS_TESTED], (uint32_t)__popcll(tm));
        }
        occluded = occluded && a.occlusion && a.phase == 1u;
        const uint64_t survM = __ballot(survives), occlM = __ballot(occluded);
        const uint32_t wv = threadIdx.x >> 6;
        __syncthreads();                                  // the previous round's slots have been read
        if ((threadIdx.x & 63u) == 0u) { waveSurv[wv] = (uint32_t)__popcll(survM); waveOccl[wv] = (uint32_t)__popcll(occlM); }
        __syncthreads();
        if (threadIdx.x < 2u) {
            const uint32_t* ws = threadIdx.x == 0u ? waveSurv : waveOccl;
            const uint32_t total = ws[0] + ws[1] + ws[2] + ws[3];
            blockSlots[threadIdx.x] = total ? atomicAdd(threadIdx.x == 0u ? tempCount : &a.counters[CNT_REPLAY_MESHLETS], total) : 0u;
        }
        __syncthreads();
        uint32_t slot = blockSlots[0] + lane_rank(survM), rs = blockSlots[1] + lane_rank(occlM);
        for (uint32_t w = 0; w < wv; w++) { slot += waveSurv[w]; rs += waveOccl[w]; }
        if (occluded) {      // (only set in phase 1 of a frame with occlusion culling)
            if (rs < a.recordCapacity) { uint4* dst = reinterpret_cast<uint4*>(&a.replayBuckets[rs]); dst[0] = againLo; dst[1] = make_uint4(againHi.x, againHi.y, 0u, 0u); }
            else atomicAdd(&a.counters[CNT_DROPPED_RECORDS], 1u);
        }
        if (survives) {
            if (slot < a.visibleCapacity) {
                TempVisible t; t.packed = packed; t.bit = bit; t.pad0 = t.pad1 = t.pad2 = 0;
                temp[slot] = t;
                atomicOr(&bitmask[bit >> 5], 1u << (bit & 31u));
                blockDirty[bit >> 16] = 1;        // (the bit's 2048-word block of the ranking; every writer stores 1)
            } else atomicAdd(&a.counters[CNT_DROPPED_CLUSTERS], 1u);
        }
    }
}

#undef BRMI_CULL_KERNEL
#undef BRMI_ST_PARAM
#undef BRMI_ST_ARG
