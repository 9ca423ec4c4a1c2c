// The optimizer step of the C ABI (include/promonet_hip.h): the gradient
// statistics with the step's control block, the AdamW update and the update
// of the loss scale. Kernels: pm_optim.h. Every argument is checked before
// the first HIP call, so the checks answer on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pm_host.h"
#include "pm_optim.h"

namespace {

static_assert(sizeof(OptTable) + sizeof(OptHyper) + 64 <= 4096,
              "the table and the other arguments must stay under the 4 KB of "
              "kernel arguments");

long long chunks_of(long long numel) {
    return (numel + OPT_CHUNK - 1) / OPT_CHUNK;
}

// What is wrong with the list, or NULL; *groups = its workgroups, *total = its
// elements
const char* check_list(const long long* numel, int count, long long* groups,
                       long long* total) {
    if (count <= 0) return "count must be at least 1";
    if (!numel) return "numel is NULL";
    *groups = *total = 0;
    for (int k = 0; k < count; ++k) {
        if (numel[k] <= 0) return "every numel must be at least 1";
        if (chunks_of(numel[k]) > PM_MAX_GRID)
            return "a tensor has too many elements for one launch";
        *groups += chunks_of(numel[k]);
        *total += numel[k];
    }
    return nullptr;
}

const char* check_grads(const void* const* grad, const int* dtype, int count) {
    if (!grad || !dtype) return "a NULL array";
    for (int k = 0; k < count; ++k) {
        if (dtype[k] != PM_F32 && dtype[k] != PM_F16 && dtype[k] != PM_BF16)
            return "dtype must be PM_F32, PM_F16 or PM_BF16";
        if (!grad[k]) return "a NULL tensor";
    }
    return nullptr;
}

OptPartials layout_of(long long groups, void* base, size_t* total) {
    PmCarve c(base);
    const size_t n = (size_t)groups;
    const OptPartials p = {c.take<float>(n), c.take<float>(n),
                           c.take<float>(n), c.take<float>(n),
                           c.take<unsigned>(n)};
    *total = c.used;
    return p;
}

// Adds an entry to the table; false when the launch is full
bool add_entry(OptTable* t, int* groups, const OptEntry& e) {
    const long long more = chunks_of(e.numel);
    if (t->count == OPT_MAX_ENTRIES || *groups + more > PM_MAX_GRID)
        return false;
    t->e[t->count] = e;
    t->e[t->count].first = *groups;
    ++t->count;
    *groups += (int)more;
    return true;
}

// Neither NaN nor +-inf, asked of the bits
bool is_finite(double x) {
    unsigned long long bits;
    memcpy(&bits, &x, sizeof bits);
    return (bits >> 52 & 0x7ff) != 0x7ff;
}

bool valid_beta(double beta) {
    return is_finite(beta) && beta >= 0. && beta < 1.;
}

bool valid_hyper(const OptHyper& h) {
    return is_finite(h.lr) && h.lr >= 0. && valid_beta(h.beta1) &&
           valid_beta(h.beta2) && is_finite(h.eps) && h.eps >= 0. &&
           is_finite(h.weight_decay) && h.weight_decay >= 0.;
}

}  // namespace

extern "C" int pm_optim_chunk(void) { return OPT_CHUNK; }

extern "C" int pm_optim_entries_per_launch(void) { return OPT_MAX_ENTRIES; }

extern "C" size_t pm_optim_workspace_bytes(const long long* numel, int count) {
    long long groups, elements;
    if (check_list(numel, count, &groups, &elements)) return 0;
    size_t total;
    layout_of(groups, nullptr, &total);
    return total;
}

extern "C" int pm_optim_grad_stats(const void* const* grad,
                                   const long long* numel, const int* dtype,
                                   int count, const float* grad_scale,
                                   const float* found_inf, double clip,
                                   double beta1, double beta2, double* state,
                                   float* stats, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    long long groups, elements;
    if (const char* why = check_list(numel, count, &groups, &elements))
        return pm_fail(PM_EINVAL, "pm_optim_grad_stats: %s", why);
    if (const char* why = check_grads(grad, dtype, count))
        return pm_fail(PM_EINVAL, "pm_optim_grad_stats: %s", why);
    if (!stats || !workspace)
        return pm_fail(PM_EINVAL, "pm_optim_grad_stats: null argument");
    if (!is_finite(clip))
        return pm_fail(PM_EINVAL, "pm_optim_grad_stats: clip is not finite");
    if (state && !(valid_beta(beta1) && valid_beta(beta2)))
        return pm_fail(PM_EINVAL,
                       "pm_optim_grad_stats: the betas must be in [0, 1)");
    size_t total;
    const OptPartials part = layout_of(groups, workspace, &total);
    if (workspace_bytes < total)
        return pm_fail(PM_EINVAL, "pm_optim_grad_stats: workspace too small");
    OptTable t;
    t.unused = 0;
    long long base = 0;
    int k = 0;
    while (k < count) {
        t.count = 0;
        t.base = base;
        int launch_groups = 0;
        for (; k < count; ++k) {
            OptEntry e = {};
            e.g = grad[k];
            e.numel = numel[k];
            e.dtype = (unsigned char)dtype[k];
            e.aligned = pm_aligned16(e.g);
            if (!add_entry(&t, &launch_groups, e)) break;
        }
        hipLaunchKernelGGL(opt_partials_kernel, dim3(launch_groups),
                           dim3(OPT_THREADS), 0, (hipStream_t)stream, t, part);
        PM_HIP_TRY(hipGetLastError());
        base += launch_groups;
    }
    hipLaunchKernelGGL(opt_final_kernel, dim3(1), dim3(OPT_THREADS), 0,
                       (hipStream_t)stream, part, groups, elements, grad_scale,
                       found_inf, clip, beta1, beta2, state, stats);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_optim_adamw_step(void* const* param, void* const* exp_avg,
                                   void* const* exp_avg_sq,
                                   const void* const* grad,
                                   const long long* numel, const int* dtype,
                                   int count, const float* stats,
                                   const double* state, double lr,
                                   double beta1, double beta2, double eps,
                                   double weight_decay, void* stream) {
    long long groups, elements;     // (of the list; the launches count theirs)
    if (const char* why = check_list(numel, count, &groups, &elements))
        return pm_fail(PM_EINVAL, "pm_optim_adamw_step: %s", why);
    if (const char* why = check_grads(grad, dtype, count))
        return pm_fail(PM_EINVAL, "pm_optim_adamw_step: %s", why);
    if (!param || !exp_avg || !exp_avg_sq)
        return pm_fail(PM_EINVAL, "pm_optim_adamw_step: a NULL array");
    for (int k = 0; k < count; ++k)
        if (!param[k] || !exp_avg[k] || !exp_avg_sq[k])
            return pm_fail(PM_EINVAL, "pm_optim_adamw_step: a NULL tensor");
    if (!stats || !state)
        return pm_fail(PM_EINVAL, "pm_optim_adamw_step: null argument");
    const OptHyper h = {lr, beta1, beta2, eps, weight_decay};
    if (!valid_hyper(h))
        return pm_fail(PM_EINVAL,
                       "pm_optim_adamw_step: lr, eps and weight_decay must be "
                       "at least 0 and the betas in [0, 1)");
    OptTable t;
    t.unused = 0;
    t.base = 0;
    int k = 0;
    while (k < count) {
        t.count = 0;
        int launch_groups = 0;
        for (; k < count; ++k) {
            OptEntry e = {};
            e.p = (float*)param[k];
            e.m = (float*)exp_avg[k];
            e.v = (float*)exp_avg_sq[k];
            e.g = grad[k];
            e.numel = numel[k];
            e.dtype = (unsigned char)dtype[k];
            e.aligned = pm_aligned16(e.p) && pm_aligned16(e.m) &&
                        pm_aligned16(e.v) && pm_aligned16(e.g);
            if (!add_entry(&t, &launch_groups, e)) break;
        }
        hipLaunchKernelGGL(opt_step_kernel, dim3(launch_groups),
                           dim3(OPT_THREADS), 0, (hipStream_t)stream, t, stats,
                           state, h);
        PM_HIP_TRY(hipGetLastError());
    }
    return PM_OK;
}

extern "C" int pm_optim_scaler_update(float* scale, int* growth_tracker,
                                      float* const* found_inf, int count,
                                      double growth, double backoff,
                                      int growth_interval, void* stream) {
    if (!scale || !growth_tracker || !found_inf)
        return pm_fail(PM_EINVAL, "pm_optim_scaler_update: null argument");
    if (count <= 0 || count > OPT_MAX_FOUND)
        return pm_fail(PM_EINVAL,
                       "pm_optim_scaler_update: count must be 1 to %d",
                       OPT_MAX_FOUND);
    OptFound found = {};
    found.count = count;
    for (int k = 0; k < count; ++k) {
        if (!found_inf[k])
            return pm_fail(PM_EINVAL, "pm_optim_scaler_update: a NULL scalar");
        found.p[k] = found_inf[k];
    }
    if (!is_finite(growth) || growth <= 1. || !is_finite(backoff) ||
        backoff <= 0. || backoff >= 1. || growth_interval <= 0)
        return pm_fail(PM_EINVAL,
                       "pm_optim_scaler_update: growth must be above 1, "
                       "backoff in (0, 1) and growth_interval at least 1");
    hipLaunchKernelGGL(opt_scaler_kernel, dim3(1), dim3(1), 0,
                       (hipStream_t)stream, scale, growth_tracker, found,
                       growth, backoff, growth_interval);
    PM_HIP_TRY(hipGetLastError());
    return PM_OK;
}
