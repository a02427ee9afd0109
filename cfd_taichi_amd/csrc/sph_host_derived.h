// sph_host_derived.h -- a SECTION of csrc/sph_mi355x.hip's one translation unit (included there once, inside its anonymous namespace, in file order):
// the host side of the derived per-particle fields (kernels in sph_derived_kernels.h).  Not a stand-alone header: it uses
// SphHandle and the helpers defined above its include.

// width in floats of a quantity and its first plane in the result; false: unknown id
inline bool derived_quantity(int which, int *width, int *first)
{
    switch (which) {
    case SPH_D_VELGRAD: *width = 9; *first = DV_VELGRAD; return true;
    case SPH_D_VORTICITY: *width = 3; *first = DV_VORTICITY; return true;
    case SPH_D_DIVERGENCE: *width = 1; *first = DV_DIVERGENCE; return true;
    case SPH_D_NORMAL: *width = 3; *first = DV_NORMAL; return true;
    case SPH_D_COVER: *width = 1; *first = DV_COVER; return true;
    }
    return false;
}

// Memory of its own (not the handle's arena), taken at the first call: a handle that never asks is laid out as before.  Per particle of the
// capacity: the packed (vel, rho) operand, the 17 planes of the result in device order, and nine floats in which a quantity is put into API order
// (the handle's staging buffer holds three)
int derived_scratch(SphHandle *h)
{
    if (h->own.derived) return SPH_OK;
    const size_t st = (size_t)h->c.stride;
    h->own.derived.want(&h->drv_vr, st);
    h->own.derived.want(&h->drv_out, kDerivedPlanes * st);
    h->own.derived.want(&h->drv_api, 9 * st);
    HIP_TRY(h, h->own.derived.commit(h->stream));
    return SPH_OK;
}

// The two launches: (vel, rho) of this solver into one array -- rho through the field table, as the diagnostics take it -- then the sweep, in the
// handle's sweep mode over the lists of the last build
int launch_derived(SphHandle *h)
{
    const Consts &c = h->c;
    FieldLoc rho;
    if (int rc = locate_field(h, SPH_F_RHO, FV_API, &rho)) return rc;
    ProfScope ps(h, K_DERIVED);
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(k_derived_pack, grid_for(c.n), dim3(kBlock), 0, s, c.n, (const float4 *)h->V[h->vcur], (const float *)rho.data, h->drv_vr);
    SPH_LAUNCH_RM0(k_derived, rigid_coupled(h), sweep_mode(h), c.n, sweep_lds(h, StageF4Src::kBytes), s, c, h->P[h->pcur], h->drv_vr, h->WP, h->nl, h->nlb,
                   h->cnt, rigid_view_or_none(h), h->stage_src, h->stage_cnt, h->drv_out);
    HIP_TRY(h, hipGetLastError());
    return SPH_OK;
}

int derived_fetch(SphHandle *h, int which, float *host, size_t n_floats)
{
    if (!host) return fail(h, SPH_E_INVALID, "sph_derived: null argument");
    if (h->slab) return fail(h, SPH_E_STATE, "sph_derived is not available on a slab handle (a ghost has no lists and its owner's sums are elsewhere)");
    int width = 0, first = 0;
    if (!derived_quantity(which, &width, &first)) return fail(h, SPH_E_INVALID, "sph_derived: unknown quantity %d", which);
    const size_t count = (size_t)width * (size_t)h->N;
    if (n_floats != count) return fail(h, SPH_E_INVALID, "sph_derived: quantity %d holds %zu floats, got %zu", which, count, n_floats);
    HIP_TRY(h, hipSetDevice(h->device));
    if (!(h->derived_valid && h->nl_valid && h->density_valid)) {      // (all three: a body step takes the lists down alone, STALE_BODY_MOVED)
        if (int rc = sph_compute_density(h)) return rc;
        if (int rc = derived_scratch(h)) return rc;
        if (int rc = launch_derived(h)) return rc;
        mark_stale(h, STALE_DERIVED_COMPUTED);
    }
    return fetch_api_order(h, [&] {
        hipLaunchKernelGGL(k_unsort_planes, grid_for(h->N), dim3(kBlock), 0, h->stream, h->N, (const float *)h->drv_out, (size_t)h->c.stride, first, width,
                           (const int *)h->id[h->icur], h->drv_api);
    }, h->drv_api, host, sizeof(float) * count);
}
