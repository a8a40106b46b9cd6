// hsr_tree.h — the hierarchical-semantic label rule and the reading of a level_sizes array, each stated ONCE (internal, not part of the
// C ABI) for hsr_eval.hip (flat, tree and leaf labels), hsr_frame_export.hip (the LOGITS picture), hsr_map_export.hip (a Gaussian's
// labels) and, the levels only, hsr_losses.hip (the tree cross-entropy).
// The rule: per tree level, the label is the LOWEST index whose fp32 softmax probability expf(x_i - max) / sum equals the largest one;
// the levels' labels form the mixed-radix tuple index idx = idx * size_l + label_l, level 0 most significant.  Its users must agree bit
// for bit (tests/test_gpu_frame_export.py, test_gpu_map_export.py, test_gpu_tree_labels_pin.py).  The device functions are
// __device__ __forceinline__, so the including file's flags apply to the inlined code — and cannot matter here: the rule is
// subtractions, expf, additions, divisions and comparisons, with NO multiply, so -ffp-contract has nothing to fuse.  hsr_eval.o is
// built with contraction and the two export units without; they give the same labels.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>

#include "../../include/hsr_eval.h"
#include "../../include/hsr_losses.h"

// The largest probability is fl(1 / sum): the maximal logit has expf(0) = 1, every other expf(x_i - max) <= 1, and rounding is
// monotone.  fl(e / sum) can equal it only when e >= 1 - 4 eps (below, e / sum is more than one rounding step under 1 / sum), which
// needs x_i - max > -1e-6 with expf's few-ulp error: other classes are skipped without changing the result.
__device__ __forceinline__ bool hsr_may_tie_max(float t) { return t >= -1e-6f; }

// lab[v] = argmax(softmax(.)) over n values for each of V independent rows (V pixels of a lane, or V = 1).  load(i, t) fills t[0..V)
// with value i of every row; one(i, v) returns value i of row v.
//   1. the maximum m, by fmaxf in index order (fmaxf drops a NaN and gives the same m in any order);
//   2. the sum s of expf(x_i - m) in index order, remembering the FIRST index that passes hsr_may_tie_max and its difference;
//   3. the lowest i with hsr_may_tie_max(x_i - m) and expf(x_i - m) / s == 1.0f / s: first index wins, like torch.argmax.
// Passes 1 and 2 take the values four at a time, the four loads issued before the first is used: one dependent load in flight per lane
// leaves a kernel waiting on latency (34.5 us for the 1200x680 K = 26 picture on an MI355X, profiles/export_bench.log; an LDS row
// likewise, EXPERIMENTS.md §12).  Step 3 starts at the remembered index — those before it fail the test that comes first — and where
// that index holds the maximum itself (dfirst == 0: expf(0) = 1 and 1.0f / s == 1.0f / s unless s is a NaN) it is the answer and
// nothing is read again; only a near tie in front of the maximum is searched.
// Label 0 where nothing qualifies: a NaN among the values makes s a NaN and every comparison false; with a +inf the differences are NaN
// (inf - inf) or -inf, with every value -inf all NaN, and none passes the bound.  A -inf beside finite values adds 0 and never wins.
template <int V, class Load, class One>
__device__ __forceinline__ void hsr_softmax_argmax(Load load, One one, int n, int (&lab)[V])
{
    constexpr int XU = 4;
    float m[V], s[V], dfirst[V], t[XU][V];
    int first[V];
#pragma unroll
    for (int v = 0; v < V; v++) { m[v] = -INFINITY; s[v] = 0.f; first[v] = -1; dfirst[v] = 0.f; }
    int i = 0;
    for (; i + XU <= n; i += XU) {
#pragma unroll
        for (int u = 0; u < XU; u++) load(i + u, t[u]);
#pragma unroll
        for (int u = 0; u < XU; u++)
#pragma unroll
            for (int v = 0; v < V; v++) m[v] = fmaxf(m[v], t[u][v]);
    }
    for (; i < n; i++) {
        load(i, t[0]);
#pragma unroll
        for (int v = 0; v < V; v++) m[v] = fmaxf(m[v], t[0][v]);
    }
    auto sum = [&](int at, const float (&tv)[V]) {
#pragma unroll
        for (int v = 0; v < V; v++) {
            const float d = tv[v] - m[v];
            s[v] += expf(d);
            const bool hit = first[v] < 0 && hsr_may_tie_max(d);
            first[v] = hit ? at : first[v];
            dfirst[v] = hit ? d : dfirst[v];
        }
    };
    for (i = 0; i + XU <= n; i += XU) {
#pragma unroll
        for (int u = 0; u < XU; u++) load(i + u, t[u]);
#pragma unroll
        for (int u = 0; u < XU; u++) sum(i + u, t[u]);
    }
    for (; i < n; i++) {
        load(i, t[0]);
        sum(i, t[0]);
    }
#pragma unroll
    for (int v = 0; v < V; v++) {
        const float pmax = 1.0f / s[v];
        lab[v] = 0;
        if (first[v] < 0) continue;      // every difference a NaN or below the bound
        if (dfirst[v] == 0.f) {          // the maximum itself
            lab[v] = s[v] == s[v] ? first[v] : 0;
            continue;
        }
        for (int k = first[v]; k < n; k++) {
            const float d = one(k, v) - m[v];
            if (hsr_may_tie_max(d) && expf(d) / s[v] == pmax) { lab[v] = k; break; }
        }
    }
}

// one row behind at(i)
template <class At> __device__ __forceinline__ int hsr_softmax_argmax(At at, int n)
{
    int lab[1];
    hsr_softmax_argmax<1>([&](int i, float (&t)[1]) { t[0] = at(i); }, [&](int i, int) { return at(i); }, n, lab);
    return lab[0];
}

// ---- host: the levels of a level_sizes array; level l takes the channels [begin[l], begin[l] + size[l]) ----
struct hsr_tree_levels {      // a kernel argument
    int n;
    int begin[16];
    int size[16];
};
static_assert(HSR_LOSS_MAX_LEVELS == 16 && HSR_EVAL_MAX_LEVELS == 16, "hsr_tree_levels holds 16 levels");

// What a caller needs to refuse a level_sizes array in its own words: the first level with fewer than one class (-1: none), the
// channels the levels take and the entries of the tuple table, saturated: once above INT_MAX it stays above every int.
struct hsr_tree_extent {
    int bad_level;
    long long sum, prod;
};

// reads sizes[0..L), 1 <= L <= 16 (the caller has checked L), and fills *lv (NULL: the extent only, for a kernel that reads the sizes
// themselves); the levels from a bad one on stay zero
inline hsr_tree_extent hsr_parse_tree_levels(int L, const int* sizes, hsr_tree_levels* lv)
{
    hsr_tree_extent e = {-1, 0, 1};
    hsr_tree_levels levels = {};
    levels.n = L;
    for (int l = 0; l < L; l++) {
        if (sizes[l] < 1) {
            e.bad_level = l;
            break;
        }
        levels.begin[l] = (int)e.sum;      // exact while the sum fits K, which every caller that reads begin requires
        levels.size[l] = sizes[l];
        e.sum += sizes[l];
        e.prod = e.prod > INT_MAX ? e.prod : e.prod * sizes[l];
    }
    if (lv) *lv = levels;
    return e;
}
