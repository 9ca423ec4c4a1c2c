// The adversarial losses of the C ABI (include/promonet_hip.h): the
// multi-tensor mean and its backward. Kernels: pm_adv.h. Every argument is
// checked before the first HIP call, so the checks answer on a machine
// without a GPU.
#include <hip/hip_runtime.h>

#include "pm_host.h"
#include "pm_adv.h"

namespace {

static_assert(sizeof(AdvTable) <= 3072, "the table must stay well under the "
                                        "4 KB of kernel arguments");

long long chunks_of(long long numel) {
    return (numel + ADV_CHUNK - 1) / ADV_CHUNK;
}

// What is wrong with the list, or NULL; *groups = its workgroups
const char* check_list(const long long* numel, int count, long long* groups) {
    if (count <= 0) return "count must be at least 1";
    if (!numel) return "numel is NULL";
    *groups = 0;
    for (int k = 0; k < count; ++k) {
        if (numel[k] <= 0) return "every numel must be at least 1";
        if (chunks_of(numel[k]) > PM_MAX_GRID)
            return "a tensor has too many elements for one launch";
        *groups += chunks_of(numel[k]);
    }
    return nullptr;
}

const char* check_entries(const void* const* a, const void* const* b,
                          const int* op, const int* dtype, int count) {
    if (!a || !op || !dtype) return "a NULL array";
    for (int k = 0; k < count; ++k) {
        if (op[k] < PM_ADV_ABS_DIFF || op[k] > PM_ADV_HINGE_ONE_PLUS)
            return "unknown op";
        if (dtype[k] != PM_F32 && dtype[k] != PM_F16 && dtype[k] != PM_BF16)
            return "dtype must be PM_F32, PM_F16 or PM_BF16";
        if (!a[k]) return "a NULL tensor";
        if (op[k] == PM_ADV_ABS_DIFF && (!b || !b[k]))
            return "PM_ADV_ABS_DIFF needs b";
    }
    return nullptr;
}

// The three parts of the workspace
struct Layout { AdvMeta* meta; double* wide; float* partials; size_t total; };

Layout layout_of(int count, long long groups, void* base) {
    PmCarve c(base);
    return {c.take<AdvMeta>(count), c.take<double>(count),
            c.take<float>((size_t)groups), c.used};
}

// Adds entry k to the table; false when the launch is full
bool add_entry(AdvTable* t, int* groups, const AdvEntry& e) {
    const long long more = chunks_of(e.numel);
    if (t->count == ADV_MAX_ENTRIES || *groups + more > PM_MAX_GRID)
        return false;
    t->e[t->count] = e;
    t->e[t->count].first = *groups;
    ++t->count;
    *groups += (int)more;
    return true;
}

}  // namespace

extern "C" int pm_multi_mean_chunk(void) { return ADV_CHUNK; }

extern "C" size_t pm_multi_mean_workspace_bytes(const long long* numel,
                                                int count) {
    long long groups;
    if (check_list(numel, count, &groups)) return 0;
    return layout_of(count, groups, nullptr).total;
}

extern "C" int pm_multi_mean(const void* const* a, const void* const* b,
                             const long long* numel, const int* op,
                             const int* dtype, int count, float* out,
                             void* workspace, size_t workspace_bytes,
                             void* stream) {
    long long groups;
    if (const char* why = check_list(numel, count, &groups))
        return pm_fail(PM_EINVAL, "pm_multi_mean: %s", why);
    if (const char* why = check_entries(a, b, op, dtype, count))
        return pm_fail(PM_EINVAL, "pm_multi_mean: %s", why);
    if (!out || !workspace)
        return pm_fail(PM_EINVAL, "pm_multi_mean: null argument");
    const Layout l = layout_of(count, groups, workspace);
    if (workspace_bytes < l.total)
        return pm_fail(PM_EINVAL, "pm_multi_mean: workspace too small");
    AdvTable t;
    long long base = 0;
    int k = 0;
    while (k < count) {
        t.count = 0;
        t.index0 = k;
        t.base = base;
        int launch_groups = 0;
        for (; k < count; ++k) {
            AdvEntry e;
            e.a = a[k];
            e.b = op[k] == PM_ADV_ABS_DIFF ? b[k] : nullptr;
            e.grad = nullptr;
            e.numel = numel[k];
            e.op = (unsigned char)op[k];
            e.dtype = (unsigned char)dtype[k];
            e.aligned = pm_aligned16(e.a) && pm_aligned16(e.b);
            e.unused = 0;
            if (!add_entry(&t, &launch_groups, e)) break;
        }
        hipLaunchKernelGGL(adv_partials_kernel, dim3(launch_groups),
                           dim3(ADV_THREADS), 0, (hipStream_t)stream, t,
                           l.partials, l.meta);
        PM_HIP_TRY(hipGetLastError());
        base += launch_groups;
    }
    hipLaunchKernelGGL(adv_final_kernel, dim3(1), dim3(ADV_FINAL_THREADS), 0,
                       (hipStream_t)stream, (const float*)l.partials,
                       (const AdvMeta*)l.meta, l.wide, count, out);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_multi_mean_backward(const void* const* a,
                                      const void* const* b,
                                      const long long* numel, const int* op,
                                      const int* dtype, int count,
                                      const float* grad_out,
                                      void* const* grad_a,
                                      void* const* grad_b, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    long long groups;
    if (const char* why = check_list(numel, count, &groups))
        return pm_fail(PM_EINVAL, "pm_multi_mean_backward: %s", why);
    if (const char* why = check_entries(a, b, op, dtype, count))
        return pm_fail(PM_EINVAL, "pm_multi_mean_backward: %s", why);
    if (!grad_out || (!grad_a && !grad_b))
        return pm_fail(PM_EINVAL, "pm_multi_mean_backward: null argument");
    for (int k = 0; k < count; ++k)
        if (op[k] == PM_ADV_ABS_DIFF && grad_a && grad_a[k])
            return pm_fail(PM_EINVAL,
                           "pm_multi_mean_backward: PM_ADV_ABS_DIFF has no "
                           "gradient for a (the real maps are constants)");
    AdvTable t;
    t.index0 = 0;
    t.base = 0;
    int k = 0;
    while (k < count) {
        t.count = 0;
        int launch_groups = 0;
        for (; k < count; ++k) {
            AdvEntry e;
            e.grad = op[k] == PM_ADV_ABS_DIFF ? (grad_b ? grad_b[k] : nullptr)
                                              : (grad_a ? grad_a[k] : nullptr);
            if (!e.grad) continue;
            e.a = a[k];
            e.b = op[k] == PM_ADV_ABS_DIFF ? b[k] : nullptr;
            e.numel = numel[k];
            e.op = (unsigned char)op[k];
            e.dtype = (unsigned char)dtype[k];
            e.aligned = pm_aligned16(e.a) && pm_aligned16(e.b) &&
                        pm_aligned16(e.grad);
            e.unused = 0;
            if (!add_entry(&t, &launch_groups, e)) break;
        }
        if (!t.count) break;
        hipLaunchKernelGGL(adv_backward_kernel, dim3(launch_groups),
                           dim3(ADV_THREADS), 0, (hipStream_t)stream, t,
                           grad_out);
        PM_HIP_TRY(hipGetLastError());
    }
    return PM_OK;
}
