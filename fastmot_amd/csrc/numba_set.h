// The probe sequence of Numba's integer set (hash(k) = k, power-of-two table), the one place it is written down in C++:
// the cascade's unmatched order (assoc.hip) and the cross-tile merge's survivor order (tilemerge.hip) both iterate such a
// table, and a correction to the probing must reach both.  Python restatement: fastmot_amd/utils/setorder.py.
#pragma once
#include <cstddef>
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
