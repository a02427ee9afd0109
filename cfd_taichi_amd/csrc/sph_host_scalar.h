// sph_host_scalar.h -- a SECTION of csrc/sph_mi355x.hip's one translation unit (included there once, inside its anonymous namespace, in file order):
// the host side of the carried scalar (kernels in sph_scalar_kernels.h).  Not a stand-alone header: it uses SphHandle and the
// helpers defined above its include.

inline bool scalar_on(const SphHandle *h) { return h->sc_T != nullptr; }

// the sweep's and the kick's constants: formed in f64 from the f32 values the sweeps use, rounded once
inline ScalarConsts scalar_consts(const SphHandle *h)
{
    const Consts &c = h->c;
    ScalarConsts k;
    k.eta2 = (float)(0.01 * (double)c.h * (double)c.h);
    k.kq = (float)(12.0 * h->sc_D * ((double)c.m / (double)c.rho0) * (double)c.kw / (double)c.h);
    k.beta = h->sc_beta;
    k.t_ref = h->sc_ref;
    return k;
}

// (x, T) of every particle in device order, then the sweep in the handle's sweep mode over the lists of the last build.  One profile entry per call.
// step_begin launches it right behind the sort and the list build: the lists and P[pcur] describe the positions the step starts from
void launch_scalar_rate(SphHandle *h)
{
    const Consts &c = h->c;
    ProfScope ps(h, K_SCALAR);
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(k_scalar_pack, grid_for(c.n), dim3(kBlock), 0, s, c.n, (const float4 *)h->P[h->pcur], (const int *)h->id[h->icur], (const float *)h->sc_T,
                       h->sc_XT);
    SPH_LAUNCH_RM0(k_scalar_rate, rigid_coupled(h), sweep_mode(h), c.n, sweep_lds(h, StageF4<>::kBytes), s, c, scalar_consts(h), (const float4 *)h->sc_XT, h->nl,
                   h->cnt, rigid_view_or_none(h), h->stage_src, h->stage_cnt, h->sc_rate);
}

// step_end, in front of the diagnostics row: the kick and T's Euler step, with dt as the step left it.  The live count, delta_time (where it is the
// host's), the buffer roles and the parameters are launch arguments: the captured wcsph step pairs are dropped whenever one of them changes
void scalar_step_end(SphHandle *h)
{
    ProfScope ps(h, K_FINALIZE);
    const bool device_dt = h->cfg.solver == SPH_SOLVER_DFSPH || h->step_adaptive;
    hipLaunchKernelGGL(k_scalar_advance, grid_for(h->c.n), dim3(kBlock), 0, h->stream, h->c.n, scalar_consts(h), StepDt{h->dt_wcsph, device_dt ? h->ds : nullptr},
                       (const DevScalars *)h->ds, (const int *)h->id[h->icur], (const float *)h->sc_rate, h->sc_T, h->V[h->vcur]);
}

int scalar_fill(SphHandle *h, int first, int m, float value)
{
    if (m <= 0) return SPH_OK;
    hipLaunchKernelGGL(k_scalar_fill, grid_for(m), dim3(kBlock), 0, h->stream, first, m, value, h->sc_T);
    HIP_TRY(h, hipGetLastError());
    return SPH_OK;
}

int scalar_refused(SphHandle *h, const char *call, bool need_on)
{
    if (h->slab) return fail(h, SPH_E_STATE, "%s is not available on a slab handle (a ghost has no lists)", call);
    if (need_on && !scalar_on(h)) return fail(h, SPH_E_STATE, "%s before sph_scalar_enable", call);
    return SPH_OK;
}

int scalar_enable(SphHandle *h, double diffusivity, double beta, double t_ref)
{
    if (int rc = scalar_refused(h, "sph_scalar_enable", false)) return rc;
    if (!std::isfinite(diffusivity) || diffusivity < 0.0) return fail(h, SPH_E_INVALID, "sph_scalar_enable: a finite diffusivity >= 0 expected, got %g", diffusivity);
    if (!std::isfinite(beta) || !std::isfinite(t_ref) || !std::isfinite((float)beta) || !std::isfinite((float)t_ref))
        return fail(h, SPH_E_INVALID, "sph_scalar_enable: finite beta and t_ref expected, got %g and %g", beta, t_ref);
    HIP_TRY(h, hipSetDevice(h->device));
    const bool fresh = !scalar_on(h);
    if (fresh) {
        // memory of its own (not the handle's arena), 24 B per particle of the capacity: XT[stride] float4, rate[stride], T[ncap]
        const size_t st = (size_t)h->c.stride;
        h->own.scalar.want(&h->sc_XT, st);
        h->own.scalar.want(&h->sc_rate, st);
        h->own.scalar.want(&h->sc_T, st);
        HIP_TRY(h, h->own.scalar.commit(h->stream));
    }
    h->sc_D = diffusivity; h->sc_beta = (float)beta; h->sc_ref = (float)t_ref;
    if (fresh) {
        h->sc_inflow = (float)t_ref;
        if (int rc = scalar_fill(h, 0, h->ncap, (float)t_ref)) return rc;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    mark_stale(h, STALE_LAUNCH_ARGS);                                // (the captured step pairs hold or lack the three launches and carry the parameters as arguments)
    return SPH_OK;
}

int scalar_disable(SphHandle *h)
{
    if (int rc = scalar_refused(h, "sph_scalar_disable", false)) return rc;
    if (!scalar_on(h)) return SPH_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    mark_stale(h, STALE_LAUNCH_ARGS);
    h->own.scalar.release();
    h->sc_XT = nullptr; h->sc_rate = h->sc_T = nullptr;
    return SPH_OK;
}

int scalar_copy(SphHandle *h, const char *call, float *down, const float *up, size_t n)
{
    if (int rc = scalar_refused(h, call, true)) return rc;
    if (!down && !up) return fail(h, SPH_E_INVALID, "%s: null argument", call);
    if (n != (size_t)h->N) return fail(h, SPH_E_INVALID, "%s: the handle holds %d particles, got %zu values", call, h->N, n);
    if (up)
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(up[i])) return fail(h, SPH_E_INVALID, "%s: value %zu is not finite", call, i);
    HIP_TRY(h, hipSetDevice(h->device));
    if (up) HIP_TRY(h, hipMemcpyAsync(h->sc_T, up, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemcpyAsync(down, h->sc_T, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SPH_OK;
}

int scalar_set_inflow(SphHandle *h, double value)
{
    if (int rc = scalar_refused(h, "sph_scalar_set_inflow", true)) return rc;
    if (!std::isfinite(value) || !std::isfinite((float)value)) return fail(h, SPH_E_INVALID, "sph_scalar_set_inflow: a finite value expected, got %g", value);
    h->sc_inflow = (float)value;
    return SPH_OK;
}

// The rate of the state the handle holds, in API order.  Builds the lists first if they are down (sph_build_neighbors; its caveat applies); changes
// neither T nor any trajectory.  The rate array is scratch between steps (every step writes it before it reads it); the handle's staging buffer
// takes the API order
int scalar_rate_fetch(SphHandle *h, float *out, size_t n)
{
    if (int rc = scalar_refused(h, "sph_scalar_rate", true)) return rc;
    if (!out) return fail(h, SPH_E_INVALID, "sph_scalar_rate: null argument");
    if (n != (size_t)h->N) return fail(h, SPH_E_INVALID, "sph_scalar_rate: the handle holds %d particles, got %zu values", h->N, n);
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->nl_valid)
        if (int rc = sph_build_neighbors(h)) return rc;
    launch_scalar_rate(h);
    return fetch_api_order(h, [&] {
        hipLaunchKernelGGL(k_scalar_unsort, grid_for(h->c.n), dim3(kBlock), 0, h->stream, h->c.n, (const float *)h->sc_rate, (const int *)h->id[h->icur], h->staging);
    }, h->staging, out, sizeof(float) * n);
}

// sph_remove_in_box / sph_geometry_carve, beside k_remove_compact and with its arguments (the roles of before the flip): the survivors' values under their new ids.
// Through the rate array, which is scratch between steps
template <class Pred>
int scalar_compact(SphHandle *h, int n, int survivors, const Pred &gone, const float4 *P, const int *id, const int *scan_id)
{
    hipLaunchKernelGGL((k_scalar_compact<Pred>), grid_for(n), dim3(kBlock), 0, h->stream, n, gone, P, id, scan_id, (const float *)h->sc_T, h->sc_rate);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->sc_T, h->sc_rate, sizeof(float) * (size_t)survivors, hipMemcpyDeviceToDevice, h->stream));
    return SPH_OK;
}
