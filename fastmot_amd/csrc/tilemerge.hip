// Cross-tile merge of a tiled detector pass, on the host.
//
// Replaces (reference file:line, relative to /root/reference)
//   SSDDetector._merge_dets / _merge    fastmot/detector.py:132-139,187-217
//   (restated in Python as SSDDetector.merge_dets, fastmot_amd/detector.py, which stays the oracle of this file)
//
// The same object seen by neighbouring tiles comes back once per tile; a detection links to every detection of the same
// class in ANOTHER tile whose intersection-over-minimum reaches the threshold, connected groups collapse into their
// first member.  Host code by design: the walk over the groups is serial, n is a few hundred rows at most and the rows
// have been read back in any case (the LAP is on the host for the same reason).
// The survivors leave in the iteration order of the reference's `keep` set -- Numba's integer set, whose table shrinks
// while detections are discarded (utils/setorder.py IntSet is the Python restatement) -- and are then ordered by class
// with a STABLE sort (the reference's np.argsort leaves the order inside a class open).
#include "common.h"
#include "numba_set.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace {

// utils/setorder.py IntSet: keys 0..n-1 with hash(k) = k in an open-addressing table of a power-of-two size >= 2 n
struct IntSet {
    static constexpr int64_t EMPTY = -1, DELETED = -2;
    static constexpr size_t MINSIZE = 16;
    std::vector<int64_t> table;
    size_t used;

    explicit IntSet(size_t n) : used(n) {
        size_t size = MINSIZE;
        while (size < 2 * n) size <<= 1;
        table.assign(size, EMPTY);
        for (size_t k = 0; k < n; ++k) table[k] = (int64_t)k;
    }
    size_t slot(int64_t k) const { return numba_set_slot(table, k); }     // (numba_set.h: shared with assoc.hip)
    void discard(int64_t k) {
        const size_t i = slot(k);
        if (table[i] != k) return;
        table[i] = DELETED;
        --used;
        size_t size = table.size();
        const size_t min_entries = std::max(2 * used, MINSIZE);
        if (4 * min_entries <= size && size > MINSIZE) {
            while ((size >> 1) >= min_entries) size >>= 1;
            std::vector<int64_t> live;
            for (int64_t v : table)
                if (v >= 0) live.push_back(v);
            table.assign(size, EMPTY);
            for (int64_t v : live) table[slot(v)] = v;
        }
    }
};

}  // namespace

extern "C" int fm_detect_merge_tiles(const fm_det48* dets, const int32_t* tile_ids, int n, int n_tiles, double thresh,
                                     fm_det48* out, int* n_out) {
    FM_CHECK_ARG(n >= 0 && n_tiles >= 1 && n_out && (n == 0 || (dets && tile_ids && out)));
    for (int i = 0; i < n; ++i) FM_CHECK_ARG(tile_ids[i] >= 0 && tile_ids[i] < n_tiles);
    *n_out = 0;
    if (n == 0) return 0;
    std::vector<double> area((size_t)n);
    for (int i = 0; i < n; ++i) {
        const double bw = dets[i].tlbr[2] - dets[i].tlbr[0] + 1, bh = dets[i].tlbr[3] - dets[i].tlbr[1] + 1;
        area[i] = (bw <= 0 || bh <= 0) ? 0. : bw * bh;
    }
    // links[i]: the running maxima of the intersection-over-minimum per neighbouring tile, scanned in index order
    std::vector<std::vector<int>> links((size_t)n);
    std::vector<double> best((size_t)n_tiles);
    for (int i = 0; i < n; ++i) {
        std::fill(best.begin(), best.end(), 0.);
        const fm_det48& a = dets[i];
        for (int j = 0; j < n; ++j) {
            const fm_det48& b = dets[j];
            if (tile_ids[j] == tile_ids[i] || b.label != a.label) continue;
            const double iw = std::min(a.tlbr[2], b.tlbr[2]) - std::max(a.tlbr[0], b.tlbr[0]) + 1;
            const double ih = std::min(a.tlbr[3], b.tlbr[3]) - std::max(a.tlbr[1], b.tlbr[1]) + 1;
            const double iom = (iw <= 0 || ih <= 0) ? 0. : iw * ih / std::min(area[i], area[j]);
            if (!(iom >= thresh)) continue;
            if (iom > best[tile_ids[j]]) {
                best[tile_ids[j]] = iom;
                links[i].push_back(j);
            }
        }
    }
    std::vector<fm_det48> work(dets, dets + n);
    std::vector<char> seen((size_t)n, 0);
    IntSet keep((size_t)n);
    std::vector<int> todo, group;
    for (int i = 0; i < n; ++i) {
        if (links[i].empty() || seen[i]) continue;
        seen[i] = 1;
        todo.assign(1, i);
        group.clear();
        while (!todo.empty()) {
            const int cur = todo.back();
            todo.pop_back();
            for (int j : links[cur])
                if (!seen[j]) {
                    seen[j] = 1;
                    group.push_back(j);
                    todo.push_back(j);
                }
        }
        for (int k : group) {
            work[i].tlbr[0] = std::min(work[i].tlbr[0], work[k].tlbr[0]);
            work[i].tlbr[1] = std::min(work[i].tlbr[1], work[k].tlbr[1]);
            work[i].tlbr[2] = std::max(work[i].tlbr[2], work[k].tlbr[2]);
            work[i].tlbr[3] = std::max(work[i].tlbr[3], work[k].tlbr[3]);
            work[i].conf = std::max(work[i].conf, work[k].conf);
            keep.discard(k);
        }
    }
    std::vector<fm_det48> kept;
    kept.reserve(keep.used);
    for (int64_t v : keep.table)
        if (v >= 0) kept.push_back(work[(size_t)v]);
    std::stable_sort(kept.begin(), kept.end(), [](const fm_det48& x, const fm_det48& y) { return x.label < y.label; });
    std::copy(kept.begin(), kept.end(), out);
    *n_out = (int)kept.size();
    return 0;
}
