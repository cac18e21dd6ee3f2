// K2's kernels — the forms of k_extend and k_extend2 that pick_extend_batch / pick_extend2 name — and their launcher.
#include "pt_k2_extend.h"

namespace pt {

typedef void (*extend_fn)(SceneD, PoolD, CountersD*);
typedef void (*extend2_fn)(SceneD, PoolD, CountersD*, uint32_t);
static extend2_fn pick_extend2(int code) {   // code = stack entries * 10 + min blocks per CU
    switch (code) {
    case 163: return k_extend2<16, 3>;
    case 164: return k_extend2<16, 4>;
    case 204: return k_extend2<20, 4>;
    case 283: return k_extend2<28, 3>;   // deep trees (the GPU builder's LBVHs of million-triangle meshes): 47.5 / 51.5 KB of LDS per block,
    case 323: return k_extend2<32, 3>;   // still three blocks per CU (160 KB)
    case 1164: return k_extend2<16, 4, 64>;    // [r3] block-size A/B (PT_EXT2): one wave per block and 512-slot windows ...
    case 2164: return k_extend2<16, 4, 128>;
    case 8164: return k_extend2<16, 4, 512>;   // ... to eight waves and 4096-slot windows
    default: return k_extend2<24, 3>;   // 24 stack entries: 43.5 KB of LDS per block, three blocks per CU
    }
}
// the MOT forms (motion in effect, pt_amd.h): the default codes only — any other code becomes the default one for its stack
static extend2_fn pick_extend2_mot(int code) {
    const int stack = (code % 1000) / 10;
    if (stack <= 16) return k_extend2<16, 4, 128, true>;
    if (stack <= 20) return k_extend2<20, 4, BLOCK, true>;
    if (stack <= 24) return k_extend2<24, 3, BLOCK, true>;
    if (stack <= 28) return k_extend2<28, 3, BLOCK, true>;
    return k_extend2<32, 3, BLOCK, true>;
}
static int extend2_threads(int code) { return code >= 1000 ? (code / 1000) * 64 : BLOCK; }
static int extend2_threads_mot(int code) { return (code % 1000) / 10 <= 16 ? 128 : BLOCK; }
static extend_fn pick_extend_batch(uint32_t flat, uint32_t pairs, bool motion = false) {
    if (motion) return !flat ? k_extend<false, false, true> : pairs ? k_extend<true, true, true> : k_extend<true, false, true>;
    return !flat ? k_extend<false, false> : pairs ? k_extend<true, true> : k_extend<true, false>;
}
void launch_extend(const SceneD& sc, const PoolD& pool, CountersD* cnt, int max_blocks, int code, hipStream_t st, bool motion, uint32_t split) {   // code: pt_render.cpp extend_code
    if (code <= -100) {
        const int kb = motion ? extend2_threads_mot(-code) : extend2_threads(-code);
        const uint32_t blocks = clamp_blocks(pool.n_alloc / (uint32_t)(EXT_WINDOW / BLOCK * kb), max_blocks);   // one per window at most
        hipLaunchKernelGGL(motion ? pick_extend2_mot(-code) : pick_extend2(-code), dim3(blocks), dim3((uint32_t)kb), 0, st, sc, pool, cnt, split);
    }
    else hipLaunchKernelGGL(pick_extend_batch(sc.tlas_flat, sc.flat_pairs, motion), grid_for(pool.n_alloc, max_blocks), dim3(BLOCK), 0, st, sc, pool, cnt);
}
int extend_occupancy_blocks(int code, bool motion) {
    if (code <= -100) return motion ? occupancy_blocks((const void*)pick_extend2_mot(-code), extend2_threads_mot(-code))
                                    : occupancy_blocks((const void*)pick_extend2(-code), extend2_threads(-code));
    return occupancy_blocks((const void*)pick_extend_batch(code <= -2, code == -3, motion), BLOCK);
}

}  // namespace pt
