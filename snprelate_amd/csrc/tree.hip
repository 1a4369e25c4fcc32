// C ABI of libsnpgpu, hierarchical clustering and the permutation test of the tree (include/snpgpu.h section 1h): what
// snpgdsHCluster and snpgdsCutTree need.  snpgpu_hclust_average is host code (R's hclust(method = "average") with its outputs);
// snpgpu_dist_perm is gnrDistPerm (src/SNPRelate.cpp:502-677) with the permutations on the device (kernels_tree.hip) and the
// sequential group pass on the host.  All argument errors, a malformed merge included, are found before any device is touched.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "host_util.h"

namespace snpgpu {
struct TreeMerge {
    int32_t start, n1, n2, parent;
    int64_t roff, ioff;
};
int launch_tree_gather(hipStream_t st, const double *src, int64_t r0, int64_t rows, int64_t n, const int32_t *leaf, const int32_t *inv, double *P);
int launch_tree_rows(hipStream_t st, const double *P, int64_t n, const TreeMerge *mg, const int32_t *leaf_parent, double *R, double *Inc,
                     double *obs);
int launch_tree_perm_light(hipStream_t st, const double *P, int64_t n, const TreeMerge *mg, const double *R, const int32_t *list,
                           int64_t n_list, int n_perm, uint64_t seed, double *d);
int launch_tree_iota(hipStream_t st, int32_t *arr, int64_t stride, int64_t n_arr);
int launch_tree_perm(hipStream_t st, int n_blocks, const double *P, int64_t n, const TreeMerge *mg, const double *R, const int4 *items,
                     int64_t n_items, uint64_t seed, int32_t *scratch, int64_t stride, double *d);
int launch_tree_stats(hipStream_t st, const TreeMerge *mg, int64_t n_merge, const double *d, int n_perm, const double *obs, double *z,
                      double *mean, double *sd);
}  // namespace snpgpu

using namespace snpgpu;

namespace {

// ms of the gather / row-sum pass, ms of the permutation kernels, launches of each, matrix elements gathered, permutations evaluated
thread_local double g_stats[6] = {0, 0, 0, 0, 0, 0};

constexpr int64_t TREE_MAX_N = int64_t(1) << 20;          // positions and offsets within a row stay far inside int32
constexpr size_t TREE_STAGE_BYTES = size_t(256) << 20;    // host rows go to the device in copies of at most this
constexpr int TREE_PERM_BLOCKS = 1024;                    // workgroups (of 4 waves) of one permutation launch
constexpr double TREE_ITEM_COST = 4e6;                    // gathers (plus draws) of one work item: a chunk of one merge's permutations
constexpr double TREE_LAUNCH_COST = 1e11;                 // ... of one launch (seconds at the measured gather rates)
constexpr int64_t TREE_LIGHT_LANES = int64_t(1) << 30;    // lanes of one launch of the light kernel
enum { T_PREP = 0, T_PERM = 1 };

// The tree of a merge matrix [n - 1][2] (R's convention) laid out for the kernels; build() validates it.
struct Tree {
    int64_t n = 0;
    std::vector<int32_t> leaf, inv, leaf_parent;          // leaf order (first column left), its inverse, the merge above each position
    std::vector<TreeMerge> mg;
    int64_t r_total = 0, i_total = 0;
    int build(const char *fn, int64_t n_, const int32_t *merge)
    {
        n = n_;
        const int64_t nm = n - 1;
        std::vector<uint8_t> leaf_used((size_t)n, 0), merge_used((size_t)nm, 0);
        std::vector<int32_t> size((size_t)nm);
        mg.assign((size_t)nm, TreeMerge{0, 0, 0, -1, 0, 0});
        for (int64_t m = 0; m < nm; m++) {
            int32_t sz[2];
            for (int c = 0; c < 2; c++) {
                const int64_t v = merge[2 * m + c];
                if (v < 0) {
                    if (-v > n) return fail(fn, "malformed merge: row " + std::to_string(m + 1) + " names a sample outside 1 ... n");
                    if (leaf_used[(size_t)(-v - 1)]++) return fail(fn, "malformed merge: sample " + std::to_string(-v) + " is merged twice");
                    sz[c] = 1;
                } else {
                    if (v == 0 || v > m) return fail(fn, "malformed merge: row " + std::to_string(m + 1) + " does not refer to an earlier row");
                    if (merge_used[(size_t)(v - 1)]++) return fail(fn, "malformed merge: row " + std::to_string(v) + " is merged twice");
                    sz[c] = size[(size_t)(v - 1)];
                    mg[(size_t)(v - 1)].parent = (int32_t)m;
                }
            }
            mg[(size_t)m].n1 = sz[0]; mg[(size_t)m].n2 = sz[1];
            size[(size_t)m] = sz[0] + sz[1];
        }
        // 2 (n - 1) distinct children out of n samples and n - 2 earlier rows: every one is used, the last row is the root
        leaf.assign((size_t)n, 0); inv.assign((size_t)n, 0); leaf_parent.assign((size_t)n, -1);
        mg[(size_t)(nm - 1)].start = 0;
        for (int64_t m = nm - 1; m >= 0; m--) {
            TreeMerge &t = mg[(size_t)m];
            t.roff = r_total; t.ioff = i_total;
            r_total += t.n1 + t.n2; i_total += t.n1;
            for (int c = 0; c < 2; c++) {
                const int32_t v = merge[2 * m + c], pos = t.start + (c ? t.n1 : 0);
                if (v < 0) { leaf[(size_t)pos] = -v - 1; inv[(size_t)(-v - 1)] = pos; leaf_parent[(size_t)pos] = (int32_t)m; }
                else mg[(size_t)(v - 1)].start = pos;
            }
        }
        return 0;
    }
};

// reference :628-664 on the z of every merge: group numbers per sample
void group_pass(const Tree &t, const double *z, double z_threshold, int32_t *group)
{
    const int64_t n = t.n, nm = n - 1;
    std::vector<uint8_t> flag((size_t)nm, 0);             // z >= threshold here or in a merge below (children have lower rows)
    for (int64_t i = 0; i < n; i++) group[i] = 1;
    for (int64_t m = 0; m < nm; m++) {
        const TreeMerge &g = t.mg[(size_t)m];
        if (!(z[m] >= z_threshold) && !flag[(size_t)m]) continue;
        flag[(size_t)m] = 1;
        if (g.parent >= 0) flag[(size_t)g.parent] = 1;
        int32_t mx = 0;
        for (int32_t i = 0; i < g.n1; i++) mx = std::max(mx, group[t.leaf[(size_t)(g.start + i)]]);
        for (int32_t i = g.n1; i < g.n1 + g.n2; i++) group[t.leaf[(size_t)(g.start + i)]] += mx;
    }
}

int dist_perm(const char *fn, const double *dist, int64_t n, int mem, const int32_t *merge, int n_perm, double z_threshold, uint64_t seed,
              double *z, int32_t *n1, int32_t *n2, int32_t *group, double *obs, double *perm_mean, double *perm_sd, int device)
{
    if (n < 2) return fail(fn, "invalid number of samples: a tree has at least two");
    if (n > TREE_MAX_N) return fail(fn, "invalid number of samples (2 ... 2^20)");
    if (n_perm < 50) return fail(fn, "n.perm >= 50 is not TRUE");
    if (!std::isfinite(z_threshold)) return fail(fn, "is.finite(z.threshold) is not TRUE");
    if (!dist || !merge || !z || !n1 || !n2 || !group) return fail(fn, "NULL argument: dist, merge, z, n1, n2 and group are required");
    if (mem != SNPGPU_HOST && mem != SNPGPU_DEVICE) return fail(fn, "invalid memory kind");
    Tree t;
    if (t.build(fn, n, merge)) return 1;
    const int64_t nm = n - 1;
    for (double &s : g_stats) s = 0;

    // the work: merges with NSub1 = 1 for the light kernel, chunks of the others' permutations in descending order of cost
    std::vector<int32_t> light;
    struct Heavy { double cost; int32_t m; };
    std::vector<Heavy> heavy;
    double gathered = 0, evaluated = 0;
    for (int64_t m = 0; m < nm; m++) {
        const TreeMerge &g = t.mg[(size_t)m];
        n1[m] = g.n1; n2[m] = g.n2;
        const double s1 = std::min(g.n1, g.n2);
        if (g.n1 + g.n2 == 2) continue;
        evaluated += n_perm;
        gathered += (double)n_perm * (s1 == 1 ? 2.0 : s1 * s1 + s1);
        if (s1 == 1) light.push_back((int32_t)m);
        else heavy.push_back({s1 * s1 + 8.0 * s1 + 16.0, (int32_t)m});
    }
    std::stable_sort(heavy.begin(), heavy.end(), [](const Heavy &a, const Heavy &b) { return a.cost > b.cost; });
    std::vector<int4> items;
    std::vector<size_t> launch_end;                        // item counts at which a launch ends
    double in_launch = 0;
    for (const Heavy &h : heavy) {
        const int chunk = (int)std::max(1.0, std::min((double)n_perm, std::floor(TREE_ITEM_COST / h.cost)));
        for (int p = 0; p < n_perm; p += chunk) {
            const int e = std::min(n_perm, p + chunk);
            const double c = h.cost * (e - p);
            if (in_launch > 0 && in_launch + c > TREE_LAUNCH_COST) { launch_end.push_back(items.size()); in_launch = 0; }
            items.push_back(make_int4(h.m, p, e, 0));
            in_launch += c;
        }
    }
    if (launch_end.empty() || launch_end.back() != items.size()) launch_end.push_back(items.size());
    size_t max_items = 0;
    for (size_t k = 0, b = 0; k < launch_end.size(); b = launch_end[k++]) max_items = std::max(max_items, launch_end[k] - b);
    const int perm_blocks = (int)std::min<size_t>(TREE_PERM_BLOCKS, (max_items + 3) / 4);

    Call c;
    if (c.open(fn, device, true)) return 1;
    hipStream_t s = c.st.s;
    const size_t nn = (size_t)n * (size_t)n;
    const int64_t stage_rows = mem == SNPGPU_HOST ? std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(TREE_STAGE_BYTES / (sizeof(double) * (size_t)n)))) : 0;
    const size_t need = sizeof(double) * (nn + (size_t)stage_rows * (size_t)n + (size_t)t.r_total + (size_t)t.i_total + (size_t)nm * (size_t)n_perm + 4 * (size_t)nm) +
                        sizeof(TreeMerge) * (size_t)nm + sizeof(int32_t) * (3 * (size_t)n + light.size() + (size_t)perm_blocks * 4 * (size_t)n) +
                        sizeof(int4) * max_items;
    size_t free_b = 0, total_b = 0;
    SNPGPU_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (need + (size_t(64) << 20) > free_b)
        return fail(fn, "the device cannot hold this call: " + std::to_string(need >> 20) + " MiB needed, " + std::to_string(free_b >> 20) + " MiB free");

    int rc = 0;
    DevBuf *dP = c.bufs.get(sizeof(double) * nn, rc);
    DevBuf *dleaf = c.bufs.get(sizeof(int32_t) * (size_t)n, rc), *dinv = c.bufs.get(sizeof(int32_t) * (size_t)n, rc);
    DevBuf *dlp = c.bufs.get(sizeof(int32_t) * (size_t)n, rc), *dmg = c.bufs.get(sizeof(TreeMerge) * (size_t)nm, rc);
    DevBuf *dR = c.bufs.get(sizeof(double) * (size_t)t.r_total, rc), *dInc = c.bufs.get(sizeof(double) * (size_t)t.i_total, rc);
    DevBuf *dd = c.bufs.get(sizeof(double) * (size_t)nm * (size_t)n_perm, rc);
    DevBuf *dout = c.bufs.get(sizeof(double) * 4 * (size_t)nm, rc);             // obs, z, mean, sd
    DevBuf *dlight = c.bufs.get(sizeof(int32_t) * light.size(), rc), *ditems = c.bufs.get(sizeof(int4) * max_items, rc);
    DevBuf *dscr = c.bufs.get(items.empty() ? 0 : sizeof(int32_t) * (size_t)perm_blocks * 4 * (size_t)n, rc);
    DevBuf *dstage = stage_rows ? c.bufs.get(sizeof(double) * (size_t)stage_rows * (size_t)n, rc) : nullptr;
    if (rc) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dleaf->p, t.leaf.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dinv->p, t.inv.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dlp->p, t.leaf_parent.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    SNPGPU_HIP_CHECK(hipMemcpyAsync(dmg->p, t.mg.data(), sizeof(TreeMerge) * (size_t)nm, hipMemcpyHostToDevice, s));
    if (!light.empty()) SNPGPU_HIP_CHECK(hipMemcpyAsync(dlight->p, light.data(), sizeof(int32_t) * light.size(), hipMemcpyHostToDevice, s));
    double *P = (double *)dP->p, *R = (double *)dR->p, *d = (double *)dd->p, *o_obs = (double *)dout->p, *o_z = o_obs + nm, *o_mean = o_z + nm,
           *o_sd = o_mean + nm;
    const TreeMerge *mg = (const TreeMerge *)dmg->p;

    // the matrix in leaf order, the row sums of every merge, obs
    if (mem == SNPGPU_DEVICE) {
        if (c.log.begin(T_PREP, s) || launch_tree_gather(s, dist, 0, n, n, (const int32_t *)dleaf->p, (const int32_t *)dinv->p, P) || c.log.end(s))
            return 1;
    } else {
        for (int64_t r0 = 0; r0 < n; r0 += stage_rows) {
            const int64_t rows = std::min(stage_rows, n - r0);
            SNPGPU_HIP_CHECK(hipMemcpyAsync(dstage->p, dist + r0 * n, sizeof(double) * (size_t)rows * (size_t)n, hipMemcpyHostToDevice, s));
            if (c.log.begin(T_PREP, s) || launch_tree_gather(s, (const double *)dstage->p, r0, rows, n, (const int32_t *)dleaf->p, (const int32_t *)dinv->p, P) ||
                c.log.end(s))
                return 1;
            SNPGPU_HIP_CHECK(hipStreamSynchronize(s));                        // the staging buffer is reused by the next rows
        }
    }
    if (c.log.begin(T_PREP, s) || launch_tree_rows(s, P, n, mg, (const int32_t *)dlp->p, R, (double *)dInc->p, o_obs) || c.log.end(s)) return 1;

    // the permutations
    for (size_t l0 = 0; l0 < light.size();) {
        const size_t cnt = std::min(light.size() - l0, (size_t)std::max<int64_t>(1, TREE_LIGHT_LANES / n_perm));
        if (c.log.begin(T_PERM, s) || launch_tree_perm_light(s, P, n, mg, R, (const int32_t *)dlight->p + l0, (int64_t)cnt, n_perm, seed, d) || c.log.end(s))
            return 1;
        l0 += cnt;
    }
    if (!items.empty()) {
        if (launch_tree_iota(s, (int32_t *)dscr->p, n, (int64_t)perm_blocks * 4)) return 1;
        for (size_t k = 0, b = 0; k < launch_end.size(); b = launch_end[k++]) {
            const size_t cnt = launch_end[k] - b;
            if (!cnt) continue;
            SNPGPU_HIP_CHECK(hipMemcpyAsync(ditems->p, items.data() + b, sizeof(int4) * cnt, hipMemcpyHostToDevice, s));
            const int blocks = (int)std::min<size_t>((size_t)perm_blocks, (cnt + 3) / 4);
            if (c.log.begin(T_PERM, s) ||
                launch_tree_perm(s, blocks, P, n, mg, R, (const int4 *)ditems->p, (int64_t)cnt, seed, (int32_t *)dscr->p, n, d) || c.log.end(s))
                return 1;
            SNPGPU_HIP_CHECK(hipStreamSynchronize(s));                        // the item list is reused by the next launch
        }
    }
    if (c.log.begin(T_PERM, s) || launch_tree_stats(s, mg, nm, d, n_perm, o_obs, o_z, o_mean, o_sd) || c.log.end(s)) return 1;
    SNPGPU_HIP_CHECK(hipMemcpyAsync(z, o_z, sizeof(double) * (size_t)nm, hipMemcpyDeviceToHost, s));
    if (obs) SNPGPU_HIP_CHECK(hipMemcpyAsync(obs, o_obs, sizeof(double) * (size_t)nm, hipMemcpyDeviceToHost, s));
    if (perm_mean) SNPGPU_HIP_CHECK(hipMemcpyAsync(perm_mean, o_mean, sizeof(double) * (size_t)nm, hipMemcpyDeviceToHost, s));
    if (perm_sd) SNPGPU_HIP_CHECK(hipMemcpyAsync(perm_sd, o_sd, sizeof(double) * (size_t)nm, hipMemcpyDeviceToHost, s));
    SNPGPU_HIP_CHECK(hipStreamSynchronize(s));
    if (c.log.sum_ms(T_PREP, &g_stats[0]) || c.log.sum_ms(T_PERM, &g_stats[1])) return 1;
    g_stats[2] = (double)c.log.count(T_PREP); g_stats[3] = (double)c.log.count(T_PERM);
    g_stats[4] = gathered; g_stats[5] = evaluated;
    group_pass(t, z, z_threshold, group);
    return 0;
}

}  // namespace

extern "C" {

int snpgpu_hclust_average(int64_t n, const double *dist, int64_t ld, int32_t *merge, double *height, int32_t *order)
{
    const char *fn = "snpgpu_hclust_average";
    if (n < 2) return fail(fn, "invalid number of samples: must have n >= 2 objects to cluster");
    if (n >= (int64_t(1) << 31)) return fail(fn, "invalid number of samples");
    if (!dist || !merge || !height || !order) return fail(fn, "NULL argument");
    if (ld < n) return fail(fn, "invalid leading dimension");
    // d(i, j), i > j, at D[i (i - 1) / 2 + j]: the lower triangle, as as.dist reads it
    std::vector<double> D((size_t)(n * (n - 1) / 2));
    for (int64_t i = 1; i < n; i++)
        for (int64_t j = 0; j < i; j++) {
            const double v = dist[i * ld + j];
            if (!std::isfinite(v)) return fail(fn, "NA/NaN/Inf in foreign function call (arg 'dist')");
            D[(size_t)(i * (i - 1) / 2 + j)] = v;
        }
    auto at = [&](int64_t a, int64_t b) -> double & { return a > b ? D[(size_t)(a * (a - 1) / 2 + b)] : D[(size_t)(b * (b - 1) / 2 + a)]; };
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<uint8_t> alive((size_t)n, 1);
    std::vector<int64_t> nn((size_t)n, -1), memb((size_t)n, 1);
    std::vector<double> dnn((size_t)n, inf);
    std::vector<int32_t> label((size_t)n);
    // the nearest neighbour of row i among the later rows; strict <: the lowest index wins a tie
    auto scan = [&](int64_t i) {
        double dm = inf;
        int64_t jm = -1;
        for (int64_t j = i + 1; j < n; j++)
            if (alive[(size_t)j] && at(j, i) < dm) { dm = at(j, i); jm = j; }
        nn[(size_t)i] = jm; dnn[(size_t)i] = dm;
    };
    for (int64_t i = 0; i < n; i++) label[(size_t)i] = (int32_t)(-(i + 1));
    for (int64_t i = 0; i + 1 < n; i++) scan(i);
    for (int64_t step = 0; step < n - 1; step++) {
        double dm = inf;
        int64_t im = -1;
        for (int64_t i = 0; i + 1 < n; i++)
            if (alive[(size_t)i] && nn[(size_t)i] >= 0 && dnn[(size_t)i] < dm) { dm = dnn[(size_t)i]; im = i; }
        if (im < 0) return fail(fn, "internal error: no pair left to merge");
        const int64_t i2 = im, j2 = nn[(size_t)im];             // i2 < j2: the merged cluster keeps row i2
        int32_t a = label[(size_t)i2], b = label[(size_t)j2];
        if ((a > 0 && b < 0) || (a > 0 && b > 0 && b < a)) std::swap(a, b);
        merge[2 * step] = a; merge[2 * step + 1] = b;
        height[step] = dm;
        label[(size_t)i2] = (int32_t)(step + 1);
        alive[(size_t)j2] = 0;
        const double mi = (double)memb[(size_t)i2], mj = (double)memb[(size_t)j2];
        for (int64_t k = 0; k < n; k++)
            if (alive[(size_t)k] && k != i2) at(i2, k) = (mi * at(i2, k) + mj * at(j2, k)) / (mi + mj);
        memb[(size_t)i2] += memb[(size_t)j2];
        for (int64_t i = 0; i + 1 < n; i++)
            if (alive[(size_t)i] && (i == i2 || nn[(size_t)i] == i2 || nn[(size_t)i] == j2)) scan(i);
    }
    // leaves with the first column of every merge to the left
    std::vector<int32_t> stack;
    stack.push_back((int32_t)(n - 1));
    int64_t k = 0;
    while (!stack.empty()) {
        const int32_t v = stack.back();
        stack.pop_back();
        if (v < 0) { order[k++] = -v; continue; }
        stack.push_back(merge[2 * (v - 1) + 1]);
        stack.push_back(merge[2 * (v - 1)]);
    }
    return 0;
}

int snpgpu_dist_perm(const double *dist, int64_t n, int mem, const int32_t *merge, int n_perm, double z_threshold, uint64_t seed, double *z,
                     int32_t *n1, int32_t *n2, int32_t *group, double *obs, double *perm_mean, double *perm_sd, int device)
{
    return dist_perm("snpgpu_dist_perm", dist, n, mem, merge, n_perm, z_threshold, seed, z, n1, n2, group, obs, perm_mean, perm_sd, device);
}

int snpgpu_gnrDistPerm(int n_dist, const double *dist, const int32_t *merge, int n_perm, double z_threshold, uint64_t seed, double *z,
                       int32_t *n1, int32_t *n2, int32_t *group, int device)
{
    const char *fn = "snpgpu_gnrDistPerm";
    if (n_dist < 2) return fail(fn, "invalid number of samples: a tree has at least two");
    if (!merge) return fail(fn, "NULL argument: merge is NULL");
    std::vector<int32_t> rows(2 * (size_t)(n_dist - 1));                 // R's matrix is column-major
    for (int64_t m = 0; m < n_dist - 1; m++) { rows[2 * m] = merge[m]; rows[2 * m + 1] = merge[m + (n_dist - 1)]; }
    return dist_perm(fn, dist, n_dist, SNPGPU_HOST, rows.data(), n_perm, z_threshold, seed, z, n1, n2, group, nullptr, nullptr, nullptr, device);
}

int snpgpu_tree_stats(double *stats)
{
    if (!stats) { set_error("snpgpu_tree_stats: stats is NULL"); return 1; }
    for (int k = 0; k < 6; k++) stats[k] = g_stats[k];
    return 0;
}

}  // extern "C"
