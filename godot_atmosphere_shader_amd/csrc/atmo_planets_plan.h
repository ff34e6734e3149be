// The PLAN of atmo_render_planets (include/atmo_planets.h; host only: no HIP call, no context): which draws of a frame's list share a launch, as a pure
// function of each draw's footprint in its target and its kernel-family key.  The MECHANISM -- the checks, the constants, the launches -- is atmo_api.hip's;
// atmo_plan_planets exposes the plan to the tests, tools/planets_plan_check.cpp runs this header alone under the host sanitizers.
// The pair test is also the overlap rule of the target batches (include/atmo_views_target.h, rules (a) and (b)): views_target_outputs calls it.
#pragma once

#include <cstdint>

namespace atmo {

// The bytes a draw may write: `rows` rows of `row_bytes`, `pitch` bytes apart, from address `base`.  rows >= 1 and 1 <= row_bytes <= pitch.
struct Footprint {
    uint64_t base;
    int64_t rows, row_bytes, pitch;
};

// True when rule (a) or rule (b) of include/atmo_views_target.h PROVES the two footprints disjoint.  Never true for two footprints that share a byte;
// exact for equal pitches whose rows do not wrap, conservative (false) otherwise.
static inline bool footprints_disjoint(const Footprint &x, const Footprint &y) {
    const bool x_first = x.base <= y.base;
    const Footprint &a = x_first ? x : y, &b = x_first ? y : x;   // A: the footprint of lower base
    // (a) the byte ranges [base, base + (rows - 1) * pitch + row_bytes) are disjoint
    if (a.base + (uint64_t)((a.rows - 1) * a.pitch + a.row_bytes) <= b.base) return true;
    // (b) one pitch P: B starts behind A's last row, or in the gap of A's rows and ends inside it (rows of one image, side by side)
    if (a.pitch == b.pitch) {
        const uint64_t d = b.base - a.base, P = (uint64_t)a.pitch, q = d / P, r = d % P;
        if (q >= (uint64_t)a.rows || (r >= (uint64_t)a.row_bytes && r + (uint64_t)b.row_bytes <= P)) return true;
    }
    return false;
}

constexpr int PLANETS_MAX_DRAWS = 64;

struct PlanetPlanIn {
    int has_tile;      // 0: the draw's launch rectangle holds no tile -- it is in no launch, and fp and key are not looked at
    uint64_t key;      // the kernel-family key: draws of one launch have equal keys
    Footprint fp;      // the launch rectangle's bytes in the draw's target
};

// launch_of[i]: the launch that holds draw i, or -1; level[i] (may be null): its level, or -1; *n_launches.  n <= PLANETS_MAX_DRAWS, chunk >= 1.
//   level(j) = 0 when no earlier draw i < j may touch j (= footprints_disjoint does not prove them apart), else 1 + the maximum level(i) over those i;
//   launches are formed level by level; within a level the keys are taken in the order in which they first appear among that level's draws, in list order;
//   within a key the draws are cut into chunks of `chunk`, in list order.
// Two draws that may touch therefore sit in different launches, the earlier draw's first; every other pair writes disjoint bytes and commutes.
static inline void planets_plan(const PlanetPlanIn *in, int n, int chunk, int *launch_of, int *level, int *n_launches) {
    int lv[PLANETS_MAX_DRAWS];
    int top = -1;
    for (int j = 0; j < n; ++j) {
        lv[j] = -1;
        launch_of[j] = -1;
        if (!in[j].has_tile) continue;
        lv[j] = 0;
        for (int i = 0; i < j; ++i)
            if (in[i].has_tile && lv[i] + 1 > lv[j] && !footprints_disjoint(in[i].fp, in[j].fp)) lv[j] = lv[i] + 1;
        if (lv[j] > top) top = lv[j];
    }
    int launches = 0;
    for (int l = 0; l <= top; ++l) {
        for (int first = 0; first < n; ++first) {
            if (lv[first] != l || launch_of[first] >= 0) continue;   // the next key of this level: that of its first draw without a launch
            int in_chunk = 0;
            for (int i = first; i < n; ++i) {
                if (lv[i] != l || launch_of[i] >= 0 || in[i].key != in[first].key) continue;
                if (in_chunk == chunk) { launches += 1; in_chunk = 0; }
                launch_of[i] = launches;
                in_chunk += 1;
            }
            launches += 1;
        }
    }
    if (level) for (int j = 0; j < n; ++j) level[j] = lv[j];
    *n_launches = launches;
}

}  // namespace atmo
