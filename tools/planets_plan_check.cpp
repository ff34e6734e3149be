// Stand-alone check of csrc/atmo_planets_plan.h, the plan of atmo_render_planets, on the CPU under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/planets_plan_check.cpp -o planets_plan_check && ./planets_plan_check
//
// 1. The pair test (rules (a) and (b) of include/atmo_views_target.h) against a brute-force byte set, on hand cases and 10 000 random rectangle sets: it
//    never calls two footprints that share a byte disjoint, and it is exact for rectangles of one image (one pitch, rows that do not wrap).
// 2. The three invariants of the plan, on the same sets:
//    ORDER   two draws that may touch are in different launches, the earlier draw's launch first;
//    LAUNCH  a launch holds 1 .. chunk draws of one key, each with a tile; a draw without a tile is in no launch; the launch indices are 0 .. n_launches - 1;
//    LEVEL   the levels are the lowest the rule allows: a draw of level l > 0 may touch an earlier draw of level l - 1 and none of a level >= l, and the
//            launches are ordered by (level, first appearance of the key in the level, chunk).
// Prints one summary line and returns 0, or the first violation and 1.
#include "../godot_atmosphere_shader_amd/csrc/atmo_planets_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

using atmo::Footprint;
using atmo::PlanetPlanIn;

static int g_failures = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);      \
            std::printf(__VA_ARGS__);                                          \
            std::printf("\n");                                                 \
            if (++g_failures > 10) std::exit(1);                               \
        }                                                                      \
    } while (0)

static bool share_a_byte(const Footprint &a, const Footprint &b) {
    std::set<uint64_t> bytes;
    for (int64_t r = 0; r < a.rows; ++r)
        for (int64_t k = 0; k < a.row_bytes; ++k) bytes.insert(a.base + (uint64_t)(r * a.pitch + k));
    for (int64_t r = 0; r < b.rows; ++r)
        for (int64_t k = 0; k < b.row_bytes; ++k)
            if (bytes.count(b.base + (uint64_t)(r * b.pitch + k))) return true;
    return false;
}

// the rectangle (x0, y0, x1, y1) of an image at `image` with `pitch` bytes a row and px bytes a pixel
static Footprint rect_of(uint64_t image, int64_t pitch, int64_t px, int x0, int y0, int x1, int y1) {
    return {image + (uint64_t)(y0 * pitch + x0 * px), y1 - y0, (x1 - x0) * px, pitch};
}

static void check_plan(const std::vector<PlanetPlanIn> &in, int chunk, const char *what) {
    const int n = (int)in.size();
    int launch_of[atmo::PLANETS_MAX_DRAWS], level[atmo::PLANETS_MAX_DRAWS], n_launches = -1;
    atmo::planets_plan(in.data(), n, chunk, launch_of, level, &n_launches);
    std::vector<std::vector<int>> members(n_launches > 0 ? n_launches : 0);
    for (int i = 0; i < n; ++i) {
        if (!in[i].has_tile) {
            CHECK(launch_of[i] == -1 && level[i] == -1, "%s: draw %d has no tile", what, i);
            continue;
        }
        CHECK(launch_of[i] >= 0 && launch_of[i] < n_launches && level[i] >= 0, "%s: draw %d launch %d of %d", what, i, launch_of[i], n_launches);
        if (launch_of[i] >= 0 && launch_of[i] < n_launches) members[launch_of[i]].push_back(i);
    }
    // ORDER
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < j; ++i) {
            if (!in[i].has_tile || !in[j].has_tile || atmo::footprints_disjoint(in[i].fp, in[j].fp)) continue;
            CHECK(launch_of[i] < launch_of[j], "%s: draws %d and %d may touch, launches %d and %d", what, i, j, launch_of[i], launch_of[j]);
        }
    // LAUNCH
    for (int l = 0; l < n_launches; ++l) {
        CHECK(!members[l].empty() && (int)members[l].size() <= chunk, "%s: launch %d holds %d draws", what, l, (int)members[l].size());
        for (int i : members[l])
            CHECK(in[i].key == in[members[l][0]].key && level[i] == level[members[l][0]], "%s: launch %d mixes keys or levels", what, l);
    }
    // LEVEL
    for (int j = 0; j < n; ++j) {
        if (!in[j].has_tile) continue;
        int want = 0;
        for (int i = 0; i < j; ++i)
            if (in[i].has_tile && !atmo::footprints_disjoint(in[i].fp, in[j].fp) && level[i] + 1 > want) want = level[i] + 1;
        CHECK(level[j] == want, "%s: draw %d level %d, the rule gives %d", what, j, level[j], want);
    }
    for (int l = 1; l < n_launches; ++l) {
        if (members[l].empty() || members[l - 1].empty()) continue;
        const int a = members[l - 1][0], b = members[l][0];
        CHECK(level[a] <= level[b], "%s: launch %d of level %d behind launch %d of level %d", what, l, level[b], l - 1, level[a]);
        if (level[a] != level[b]) continue;
        if (in[a].key == in[b].key) {   // the next chunk of one key: the earlier one is full, and all of it comes first in the list
            CHECK((int)members[l - 1].size() == chunk && members[l - 1].back() < b, "%s: launches %d and %d split one key early", what, l - 1, l);
        } else {   // the next key: its first draw comes behind the first draw of the level with the earlier key
            int first_a = a;
            for (int i = 0; i < n; ++i) if (in[i].has_tile && level[i] == level[a] && in[i].key == in[a].key) { first_a = i; break; }
            CHECK(first_a < b, "%s: launch %d's key appears in front of launch %d's", what, l, l - 1);
            for (int k = 0; k < l; ++k)
                if (!members[k].empty() && level[members[k][0]] == level[b])
                    CHECK(in[members[k][0]].key != in[b].key, "%s: key of launch %d was closed at launch %d", what, l, k);
        }
    }
}

int main() {
    // ---- hand cases of the pair test ----
    const uint64_t img = 0x100000;
    const int64_t px = 8, pitch = 128 * px;
    const Footprint left = rect_of(img, pitch, px, 0, 0, 64, 36), right = rect_of(img, pitch, px, 64, 0, 128, 36);
    CHECK(atmo::footprints_disjoint(left, right) && atmo::footprints_disjoint(right, left), "the halves of a double-wide image");
    CHECK(!atmo::footprints_disjoint(left, rect_of(img, pitch, px, 63, 0, 128, 36)), "halves one pixel too wide");
    CHECK(!atmo::footprints_disjoint(left, left), "a footprint and itself");
    CHECK(atmo::footprints_disjoint(rect_of(img, pitch, px, 0, 0, 128, 18), rect_of(img, pitch, px, 0, 18, 128, 36)), "two row bands");
    CHECK(atmo::footprints_disjoint(rect_of(img, pitch, px, 10, 10, 20, 20), rect_of(img, pitch, px, 20, 5, 30, 25)), "side by side in one image");
    CHECK(!atmo::footprints_disjoint(rect_of(img, pitch, px, 10, 10, 20, 20), rect_of(img, pitch, px, 19, 19, 30, 25)), "one shared pixel");
    CHECK(atmo::footprints_disjoint(rect_of(img, pitch, px, 10, 10, 20, 20), rect_of(img, pitch, px, 5, 20, 30, 25)), "below");
    CHECK(atmo::footprints_disjoint(rect_of(img, pitch, px, 0, 0, 4, 4), rect_of(img + 0x100000, 64, 4, 0, 0, 4, 4)), "two images");
    CHECK(!atmo::footprints_disjoint(rect_of(img, 64, 4, 0, 0, 4, 8), rect_of(img + 16, 96, 4, 0, 0, 4, 8)),
          "interleaved rows of different pitches: conservative");

    // ---- random rectangle sets ----
    std::mt19937 rng(20240607u);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
    long pairs = 0, disjoint_pairs = 0, exact_pairs = 0, sets_with_touch = 0, launches_total = 0;
    const int sets = 10000;
    for (int s = 0; s < sets; ++s) {
        const int n = rnd(1, 12);
        const int layout = s % 4;   // 0, 1: rectangles of one image; 2: of two images of different pitches; 3: arbitrary footprints (wrapping rows too)
        const int W = rnd(8, 24), H = rnd(4, 12), pxb = 1 << rnd(0, 2);
        const int64_t p0 = (int64_t)(W + rnd(0, 5)) * pxb, p1 = (int64_t)(W + rnd(6, 9)) * pxb;
        std::vector<PlanetPlanIn> in;
        std::vector<bool> one_image_rect;
        for (int i = 0; i < n; ++i) {
            PlanetPlanIn d;
            d.has_tile = rnd(0, 9) != 0;
            d.key = (uint64_t)rnd(0, 2);
            if (layout == 3) {
                const int64_t pt = rnd(4, 40), rb = rnd(1, (int)pt);
                d.fp = {0x1000u + (uint64_t)rnd(0, 200), rnd(1, 6), rb, pt};
            } else {
                const int x0 = rnd(0, W - 1), y0 = rnd(0, H - 1), x1 = rnd(x0 + 1, W), y1 = rnd(y0 + 1, H);
                const bool second = layout == 2 && rnd(0, 1);
                // (the second image starts inside the first one's bytes, so rectangles of the two can share bytes)
                d.fp = rect_of(second ? 0x1000u + (uint64_t)(pxb * rnd(0, 40)) : 0x1000u, second ? p1 : p0, pxb, x0, y0, x1, y1);
            }
            one_image_rect.push_back(layout < 2);
            in.push_back(d);
        }
        bool any_touch = false;
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < j; ++i) {
                const bool shared = share_a_byte(in[i].fp, in[j].fp), proved = atmo::footprints_disjoint(in[i].fp, in[j].fp);
                CHECK(proved == atmo::footprints_disjoint(in[j].fp, in[i].fp), "set %d: the pair test is not symmetric (%d, %d)", s, i, j);
                CHECK(!(proved && shared), "set %d: draws %d and %d share a byte and were called disjoint", s, i, j);
                if (one_image_rect[i] && one_image_rect[j]) {
                    CHECK(proved == !shared, "set %d: rectangles %d and %d of one image: proved %d, shared %d", s, i, j, (int)proved, (int)shared);
                    exact_pairs += 1;
                }
                pairs += 1;
                disjoint_pairs += proved ? 1 : 0;
                if (!proved && in[i].has_tile && in[j].has_tile) any_touch = true;
            }
        sets_with_touch += any_touch ? 1 : 0;
        for (int chunk : {8, 1, 3}) check_plan(in, chunk, "random set");
        int launch_of[atmo::PLANETS_MAX_DRAWS], nl = 0;
        atmo::planets_plan(in.data(), n, 8, launch_of, nullptr, &nl);
        launches_total += nl;
    }
    // ---- hand cases of the plan ----
    {
        std::vector<PlanetPlanIn> in;
        for (int i = 0; i < 9; ++i) in.push_back({1, 7u, rect_of(img, pitch, px, 10 * i, 0, 10 * i + 10, 10)});   // nine disjoint boxes of one family
        int lo[64], nl = 0;
        atmo::planets_plan(in.data(), 9, 8, lo, nullptr, &nl);
        CHECK(nl == 2 && lo[7] == 0 && lo[8] == 1, "nine disjoint boxes: %d launches", nl);
        check_plan(in, 8, "nine disjoint");
        in.clear();
        for (int i = 0; i < 3; ++i) in.push_back({1, 7u, rect_of(img, pitch, px, 4 * i, 4 * i, 4 * i + 10, 4 * i + 10)});   // a chain A under B under C
        atmo::planets_plan(in.data(), 3, 8, lo, nullptr, &nl);
        CHECK(nl == 3 && lo[0] == 0 && lo[1] == 1 && lo[2] == 2, "a chain: %d launches", nl);
        in.clear();
        in.push_back({1, 1u, rect_of(img, pitch, px, 0, 0, 10, 10)});
        in.push_back({1, 2u, rect_of(img, pitch, px, 20, 0, 30, 10)});
        in.push_back({0, 1u, {0, 0, 0, 0}});
        in.push_back({1, 1u, rect_of(img, pitch, px, 40, 0, 50, 10)});
        atmo::planets_plan(in.data(), 4, 8, lo, nullptr, &nl);
        CHECK(nl == 2 && lo[0] == 0 && lo[1] == 1 && lo[2] == -1 && lo[3] == 0, "two families, one draw without a tile: %d launches", nl);
        check_plan(in, 8, "two families");
        std::vector<PlanetPlanIn> full;
        for (int i = 0; i < 64; ++i) full.push_back({1, (uint64_t)(i % 3), rect_of(img, pitch, px, (i % 8) * 12, (i / 8) * 3, (i % 8) * 12 + 14, (i / 8) * 3 + 4)});
        check_plan(full, 8, "64 draws");
        atmo::planets_plan(nullptr, 0, 8, lo, nullptr, &nl);
        CHECK(nl == 0, "no draws");
    }
    if (g_failures) return 1;
    std::printf("planets_plan_check: ok -- %d random sets, %ld pairs (%ld proved disjoint, %ld held to the exact byte set), %ld sets with a touching pair, "
                "%ld launches planned\n", sets, pairs, disjoint_pairs, exact_pairs, sets_with_touch, launches_total);
    return 0;
}
