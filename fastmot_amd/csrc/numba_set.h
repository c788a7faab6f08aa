// The probe sequence of Numba's integer set (hash(k) = k, power-of-two table), the one place it is written down in C++:
// the cascade's unmatched order (assoc.hip) and the cross-tile merge's survivor order (tilemerge.hip) both iterate such a
// table, and a correction to the probing must reach both.  fastmot_amd/utils/setorder.py documents the container; its
// unmatched_order calls numba_difference_order below (fm_unmatched_order), its IntSet restates the probing in Python.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// The slot of `table` (entries >= 0: keys, -1: empty, anything else: deleted) that holds k, or the empty slot k's probe
// sequence ends on: the home slot k & mask, three linear steps, then index = 5 index + 1 + (perturb >>= 5).
template <typename V>
inline size_t numba_set_slot(const std::vector<V>& table, V k) {
    const size_t mask = table.size() - 1;
    size_t index = (size_t)k & mask, perturb = (size_t)k;
    for (int probes = 0;; ++probes) {
        const V v = table[index];
        if (v == k || v == (V)-1) return index;
        if (probes < 3) {
            index = (index + 1) & mask;
        } else {
            perturb >>= 5;
            index = (index * 5 + 1 + perturb) & mask;
        }
    }
}

// list(set(range(n)) - set(matched)) as Numba's integer set iterates it (utils/matching.py:58-60; closed form derived in
// fastmot_amd/utils/setorder.py): gone[k] != 0 marks the matched keys.
inline void numba_difference_order(int n, const std::vector<uint8_t>& gone, std::vector<int>& out) {
    out.clear();
    for (int k = 0; k < n; ++k)
        if (!gone[k]) out.push_back(k);
    int size = 16;
    while (size < 2 * n) size <<= 1;
    const int min_entries = std::max(2 * (int)out.size(), 16);
    if (4 * min_entries > size || size <= 16) return;
    while ((size >> 1) >= min_entries) size >>= 1;
    const int mask = size - 1;
    if (out.empty() || out.back() <= mask) return;
    std::vector<int> table(size, -1);
    for (int k : out) table[numba_set_slot(table, k)] = k;
    out.clear();
    for (int k : table)
        if (k >= 0) out.push_back(k);
}
