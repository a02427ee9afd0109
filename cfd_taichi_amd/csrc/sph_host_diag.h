// sph_host_diag.h -- a SECTION of csrc/sph_mi355x.hip's one translation unit (included there once, inside its anonymous namespace, in file order):
// the host side of the run diagnostics (kernels in sph_diag_kernels.h).  Not a stand-alone header: it uses SphHandle and the
// helpers defined above its include.

constexpr int kDiagMaxRows = 1 << 20;        // 256 MiB of ring: anything larger is a mistake, not a request

// the scratch of both uses: kDiagParts partial rows and the on-demand row behind them.  Memory of its own (not the handle's arena), taken at the first
// use: a handle that never asks for diagnostics is laid out as before
int diag_scratch(SphHandle *h)
{
    if (h->own.diag) return SPH_OK;
    h->own.diag.want(&h->diag_part, (size_t)kDiagParts * kDiagPartStride);
    h->own.diag.want(&h->diag_row, kDiagSlots);
    HIP_TRY(h, h->own.diag.commit(h->stream));
    return SPH_OK;
}

// The two launches.  ctl == null: on demand, into `out`, the host's step counter as an argument; else a recorded step, which decides on the device
// whether it is due and where its row goes.  rho == null: the row carries no densities (slots 24-26 are NaN).  The live count, delta_time (where it
// is the host's) and the buffer roles are launch arguments: the captured wcsph step pairs are dropped whenever one of them changes
void launch_diag(SphHandle *h, const float *rho, DiagCtl *ctl, double *out)
{
    const int parts = std::max(1, std::min(h->nblocks, kDiagParts));
    const bool device_dt = h->cfg.solver == SPH_SOLVER_DFSPH || h->step_adaptive;
    const DiagFinal f{h->c.n, parts, (double)h->c.m, StepDt{h->dt_wcsph, device_dt ? h->ds : nullptr}, h->simulate_cnt, rho ? 1 : 0};
    hipLaunchKernelGGL(k_diag_partials, dim3((unsigned)parts), dim3(kBlock), 0, h->stream, h->c.n, (const float4 *)h->P[h->pcur], (const float4 *)h->V[h->vcur],
                       (const int *)h->id[h->icur], rho, (const DevScalars *)h->ds, (const DiagCtl *)ctl, h->diag_part);
    hipLaunchKernelGGL(k_diag_final, dim3(1), dim3(kBlock), 0, h->stream, f, (const DevScalars *)h->ds, ctl, (const double *)h->diag_part, out);
}

// the solver's rho through the field table (every solver keeps it; a solver that did not would answer here)
int diag_rho(SphHandle *h, const float **rho)
{
    FieldLoc f;
    if (int rc = locate_field(h, SPH_F_RHO, FV_API, &f)) return rc;
    *rho = (const float *)f.data;
    return SPH_OK;
}

// step_end, while recording is on: the row of the state the step leaves -- the new positions and velocities, the advanced clock, the dt it used and
// the densities its density sweep computed (pbf: its lambda sweep).  Enqueued like any launch: no host wait, nodes of the captured wcsph step pair
int diag_step_end(SphHandle *h)
{
    const float *rho = nullptr;
    if (int rc = diag_rho(h, &rho)) return rc;
    ProfScope ps(h, K_FINALIZE);
    launch_diag(h, rho, h->diag_ctl, h->diag_ring);
    return SPH_OK;
}

int diag_refused(SphHandle *h, const char *call)
{
    if (h->slab) return fail(h, SPH_E_STATE, "%s is not available on a slab handle (the sums would need an all-reduce)", call);
    return SPH_OK;
}
