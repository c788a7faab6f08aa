// Stand-alone driver for the context-free half of the association cascade (fastmot_amd/csrc/assoc.hip with lap_host.hip:
// fm_cascade_host, fm_stage_cost_host, fm_unmatched_order), meant to be built with the host sanitizers and run on the
// CPU -- no GPU, no Python:
//
//   F="--offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined"
//   hipcc $F -c fastmot_amd/csrc/assoc.hip -o /tmp/cha.o && hipcc $F -c fastmot_amd/csrc/lap_host.hip -o /tmp/chl.o
//   hipcc $F -c -x hip scripts/cascade_host_check.cpp -o /tmp/chc.o
//   /opt/rocm/llvm/bin/clang++ -fsanitize=address,undefined /tmp/cha.o /tmp/chl.o /tmp/chc.o -L/opt/rocm/lib -lamdhip64 \
//         -Wl,-rpath,/opt/rocm/lib -o /tmp/cascade_host_check && /tmp/cascade_host_check
//
// The cascade writes its output through a raw pointer; `out` here is a heap block of EXACTLY the documented minimum
// (FM_CASCADE_HEADER + 3 * (n_conf + n_unconf) + 3 * nD words) and every input array a heap block of exactly its size,
// so a store or load past either is a heap overflow the sanitizer reports.  Seeded cases with ties, gated pairs, label
// mismatches, empty groups, history rows, both transposed shapes, and the two empty sides (no detections, no rows), which
// get null pointers for the terms and labels they have no use for.
// Checked beside the bounds: the lists partition rows and detections.  Exit status 0 and "ok" when every call returned 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>
#include "../include/fastmot_hip.h"

void fm_set_error(const char*, ...) {}      // (ctx.hip's, which the library links)

#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            fprintf(stderr, "%s:%d failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                \
        }                                                            \
    } while (0)

static uint32_t rng_state = 2026;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }
static int below(int n) { return (int)((rnd() >> 8) % (uint32_t)n); }
static double unit() { return (rnd() >> 8) / 16777216.; }

template <typename T>
static T* exact(const std::vector<T>& v) {      // a heap block of exactly the vector's size (null for an empty one)
    if (v.empty()) return nullptr;
    T* p = (T*)malloc(v.size() * sizeof(T));
    memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static int run_case(int nT, int nD, bool quantise) {
    const size_t mat = (size_t)nT * nD;
    std::vector<double> feat(mat), maha(mat), iou(mat), det_conf(nD);
    for (size_t i = 0; i < mat; ++i) {
        feat[i] = 1.2 * unit(), maha[i] = 14. * unit(), iou[i] = unit();
        if (quantise) feat[i] = (int)(feat[i] * 10) / 10., maha[i] = (int)maha[i], iou[i] = (int)(iou[i] * 10) / 10.;
    }
    const int n_lab = 1 + below(3);
    std::vector<uint8_t> has_feat(nT), docc(nD);
    std::vector<int64_t> tlab(nT), dlab(nD);
    for (int t = 0; t < nT; ++t) has_feat[t] = unit() < 0.9, tlab[t] = below(n_lab);
    for (int d = 0; d < nD; ++d) docc[d] = unit() < 0.2, dlab[d] = below(n_lab), det_conf[d] = 0.3 + 0.7 * unit();
    // rows: a random permutation split into history, unconfirmed and four depth groups (the second one often empty)
    std::vector<int32_t> perm(nT);
    std::iota(perm.begin(), perm.end(), 0);
    for (int i = nT - 1; i > 0; --i) std::swap(perm[i], perm[below(i + 1)]);
    const int n_hist = nT ? below(nT / 3 + 1) : 0, n_unconf = nT ? below((nT - n_hist) / 4 + 1) : 0;
    std::vector<int32_t> hist(perm.begin(), perm.begin() + n_hist), unconf(perm.begin() + n_hist, perm.begin() + n_hist + n_unconf);
    std::vector<int32_t> conf, group_off(5, 0);
    std::vector<std::vector<int32_t>> groups(4);
    const bool hole = unit() < 0.3;
    for (int i = n_hist + n_unconf; i < nT; ++i) {
        int g = below(4);
        if (hole && g == 1) g = 2;
        groups[g].push_back(perm[i]);
    }
    for (int g = 0; g < 4; ++g) {
        conf.insert(conf.end(), groups[g].begin(), groups[g].end());
        group_off[g + 1] = (int32_t)conf.size();
    }
    std::vector<uint8_t> active(conf.size());
    for (auto& a : active) a = unit() < 0.7;
    std::vector<int64_t> hist_labels(n_hist);
    for (auto& l : hist_labels) l = below(n_lab);

    fm_cascade_in in;
    memset(&in, 0, sizeof in);
    in.n_groups = 4, in.n_unconf = n_unconf, in.n_hist = n_hist;
    in.group_off = exact(group_off), in.conf_rows = exact(conf), in.conf_active = exact(active);
    in.unconf_rows = exact(unconf), in.hist_rows = exact(hist), in.hist_labels = exact(hist_labels), in.det_conf = exact(det_conf);
    const double costs[] = {0.8, 0.9, 0.5}, ious[] = {0.6, 0.3}, reids[] = {0.6, 0.45, 0.2};
    in.motion_weight = 0.2, in.max_assoc_cost = costs[below(3)], in.fill_val = in.max_assoc_cost + 0.1 < 1. ? in.max_assoc_cost + 0.1 : 1.;
    in.max_iou_cost = ious[below(2)], in.conf_thresh = 0.5, in.max_reid_cost = reids[below(3)];
    // an empty side has no terms and no labels: null pointers, so that a read of any of them is reported
    double *pf = exact(feat), *pm = exact(maha), *pi = exact(iou);
    uint8_t *ph = mat ? exact(has_feat) : nullptr, *po = exact(docc);
    int64_t *pt = mat ? exact(tlab) : nullptr, *pd = mat ? exact(dlab) : nullptr;

    const int n_trk = (int)conf.size() + n_unconf, cap = FM_CASCADE_HEADER + 3 * n_trk + 3 * nD;
    int32_t* out = (int32_t*)malloc(sizeof(int32_t) * cap);
    CHECK(fm_cascade_host(nT, nD, pf, pm, pi, ph, pt, pd, po, &in, out, cap - 1) != 0);        // one word short: refused
    CHECK(fm_cascade_host(nT, nD, pf, pm, pi, ph, pt, pd, po, &in, out, cap) == 0);
    const int n_match = out[0] + out[1] + out[2], n_un = out[3] + out[4] + out[5];
    CHECK(out[9] <= cap && out[9] == FM_CASCADE_HEADER + 2 * n_match + n_un + 2 * out[6] + out[7] + out[8]);
    CHECK(n_match + n_un == n_trk);                             // every confirmed / unconfirmed row is matched or unmatched
    std::vector<int> row_seen(nT, 0), det_seen(nD, 0);
    const int32_t* w = out + FM_CASCADE_HEADER;
    for (int k = 0; k < n_match; ++k, w += 2) {
        CHECK(w[0] >= 0 && w[0] < nT && w[1] >= 0 && w[1] < nD);
        ++row_seen[w[0]], ++det_seen[w[1]];
    }
    for (int k = 0; k < n_un; ++k, ++w) {
        CHECK(*w >= 0 && *w < nT);
        ++row_seen[*w];
    }
    for (int k = 0; k < out[6]; ++k, w += 2) {
        CHECK(w[0] >= 0 && w[0] < n_hist && w[1] >= 0 && w[1] < nD && !docc[w[1]]);
        ++det_seen[w[1]];
    }
    for (int k = 0; k < out[7] + out[8]; ++k, ++w) {
        CHECK(*w >= 0 && *w < nD && det_conf[*w] >= in.conf_thresh && (k < out[7]) == (docc[*w] != 0));
        ++det_seen[*w];
    }
    for (int32_t r : conf) CHECK(row_seen[r] == 1);
    for (int32_t r : unconf) CHECK(row_seen[r] == 1);
    for (int d = 0; d < nD; ++d) CHECK(det_seen[d] <= 1);
    if (nT == 0) CHECK(n_match == 0 && n_un == 0 && out[6] == 0);
    if (nD == 0) CHECK(n_match == 0 && out[6] + out[7] + out[8] == 0);

    // the host fill on exactly-sized blocks, every stage, rows and columns in reverse order
    if (mat) {
        std::vector<int32_t> rows(nT), cols(nD);
        for (int t = 0; t < nT; ++t) rows[t] = nT - 1 - t;
        for (int d = 0; d < nD; ++d) cols[d] = nD - 1 - d;
        int32_t *pr = exact(rows), *pc = exact(cols);
        double* cost = (double*)malloc(sizeof(double) * mat);
        for (int stage = FM_STAGE_MATCHING; stage <= FM_STAGE_REID; ++stage) {
            CHECK(fm_stage_cost_host(stage, nT, nD, pf, pm, pi, ph, pd, po, nT, pr, nD, pc, pt, in.motion_weight,
                                     in.max_assoc_cost, in.fill_val, cost) == 0);
            for (size_t i = 0; i < mat; ++i) CHECK(cost[i] >= 0. && cost[i] <= 1e5);
        }
        free(pr), free(pc), free(cost);
    }
    // fm_unmatched_order: out of exactly n words
    {
        const int n = nT + nD;
        std::vector<int32_t> matched;
        for (int k = 0; k < n; ++k)
            if (unit() < 0.8) matched.push_back(k);
        int32_t *pmch = exact(matched), *order = (int32_t*)malloc(sizeof(int32_t) * (n ? n : 1));
        CHECK(fm_unmatched_order(n, pmch, (int)matched.size(), order) == n - (int)matched.size());
        free(pmch), free(order);
    }
    free((void*)in.group_off), free((void*)in.conf_rows), free((void*)in.conf_active), free((void*)in.unconf_rows);
    free((void*)in.hist_rows), free((void*)in.hist_labels), free((void*)in.det_conf);
    free(pf), free(pm), free(pi), free(ph), free(po), free(pt), free(pd), free(out);
    return 0;
}

int main() {
    const int sizes[][2] = {{1, 1}, {3, 7}, {7, 3}, {8, 9}, {17, 16}, {20, 50}, {50, 20}, {33, 31}, {64, 70}, {90, 40},
                            {12, 0}, {0, 13}, {0, 0}, {1, 0}, {0, 1}};       // (the empty sides last)
    for (auto& s : sizes)
        for (int rep = 0; rep < 6; ++rep)
            if (run_case(s[0], s[1], rep & 1)) {
                fprintf(stderr, "case nT=%d nD=%d rep=%d\n", s[0], s[1], rep);
                return 1;
            }
    puts("ok");
    return 0;
}
