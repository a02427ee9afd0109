// sph_host_fields.h -- a SECTION of csrc/sph_mi355x.hip's one translation unit (included there once, inside its anonymous namespace, in file order):
// which array of a handle plays which role on which solver, and the table of the fluid fields that sph_upload, sph_download, sph_download_local and the
// pbf carry of sph_build_neighbors read.  Not a stand-alone header: it uses SphHandle and the helpers defined above its include.

inline bool rigid_binned(const SphHandle *h);       // sph_host_rigid.h

// ---------------------------------------------------------------------------------------------
// Roles.  SphHandle::X[0..4], aux and VA[0] are shared storage; these are the only places that say what a solver keeps in them
// ---------------------------------------------------------------------------------------------
struct PciFields { float4 *ext_force, *press_force, *pos_predict, *press[2]; };       // press[k].w = press_iter, ping-pong (pb_final: the last step's)
inline PciFields pci_fields(const SphHandle *h) { return {h->X[0], h->X[1], h->X[2], {h->X[3], h->X[4]}}; }
struct IiFields { float4 *d_ii, *d_ij, *f_press, *p[2], *v_adv; float *a_ii; };       // p[k].w = p_iter, ping-pong (pb_final); p_past is the carried scalar
inline IiFields ii_fields(const SphHandle *h) { return {h->X[0], h->X[1], h->X[2], {h->X[3], h->X[4]}, h->VA[0], h->aux}; }
struct PbfFields { float4 *delta_pos, *pos_new, *vel_1; float *lambda; };             // pos_new / vel_1: phase 1's results, scratch between steps
inline PbfFields pbf_arrays(const SphHandle *h) { return {h->X[0], h->X[1], h->X[2], h->aux}; }
inline float *dfsph_alpha(const SphHandle *h) { return h->aux; }
inline float *wcsph_pressure(const SphHandle *h) { return h->aux; }
// what the density sweep writes beside rho (k_density): alpha on dfsph, pressure on every other solver -- iisph overwrites it with a_ii (k_ii_rho_adv)
inline float *density_aux(const SphHandle *h) { return h->aux; }

// ---------------------------------------------------------------------------------------------
// The fluid fields, SPH_F_POS .. SPH_F_PBF_DELTA_POS
// ---------------------------------------------------------------------------------------------
enum FieldKind { FK_XYZ, FK_SCALAR, FK_W, FK_COUNT, FK_INT };      // xyz / w of a float4 array, a float array, the packed list counts (cnt), an int array
enum FieldView { FV_API, FV_LOCAL };                               // sph_download / sph_upload (API order, N particles) | sph_download_local (device order, resident ones)
enum FieldState { FS_ANY, FS_STEPPED, FS_PBF_IN_ORDER };           // always | after the first step | pbf_fields: written by a step, in the current device order
enum : unsigned { SW = 1u << SPH_SOLVER_WCSPH, SD = 1u << SPH_SOLVER_DFSPH, SP = 1u << SPH_SOLVER_PCISPH, SI = 1u << SPH_SOLVER_IISPH, SB = 1u << SPH_SOLVER_PBF,
                  S_ALL = SW | SD | SP | SI | SB };

struct FieldRow {
    int field;
    FieldKind kind;
    const void *(*at)(const SphHandle *);      // where the data is now
    unsigned owners;                           // FV_API: the solvers that have it; the others answer SPH_E_STATE with `not_owner`
    const char *not_owner;
    unsigned local;                            // FV_LOCAL: the solvers sph_download_local offers it on; the others answer SPH_E_INVALID
    unsigned upload;                           // sph_upload: 0 = read-only, else the solvers that take it
    FieldState api_state, local_state;         // refused with SPH_E_STATE until it holds
};

// Where the two views disagree (kept as found; a later change may decide about each):
//   acc          sph_download: wcsph only.            sph_download_local: every solver but dfsph (VA[0], whatever it holds there -- iisph: v_adv)
//   pressure     sph_download: wcsph only.            sph_download_local: every solver but dfsph (aux -- iisph: a_ii, pbf: pbf_lambda)
//   vel_adv      sph_download: dfsph and iisph.       sph_download_local: dfsph only
//   pos_predict  sph_download: pcisph, and pbf at any time (it is pos).   sph_download_local: pbf only, and only while pbf_fields holds
//   pbf_lambda, pbf_delta_pos   sph_download: from the first step on (one GPU: carried through re-sorts; after sph_add_particles / sph_remove_in_box the rows
//                that came or moved hold what k_append / the compaction left).   sph_download_local: only while pbf_fields holds, so not after those calls either
//   nbr_count, press_iter, press_force, d_ii, a_ii, d_ij     sph_download only
#define AT(expr) [](const SphHandle *h) -> const void * { return expr; }
const FieldRow kFluidFields[] = {
    //  field               kind        where                                      sph_download: owners, refusal                                                       local         upload  state: api, local
    {SPH_F_POS,           FK_XYZ,    AT(h->P[h->pcur]),                           S_ALL,   nullptr,                                                                    S_ALL,        S_ALL,  FS_ANY, FS_ANY},
    {SPH_F_VEL,           FK_XYZ,    AT(h->V[h->vcur]),                           S_ALL,   nullptr,                                                                    S_ALL,        S_ALL,  FS_ANY, FS_ANY},
    {SPH_F_ACC,           FK_XYZ,    AT(h->VA[0]),                                SW,      "acc is a wcsph field (the other solvers never fill it, dfsph_solver.py:418-421)", S_ALL & ~SD, 0,      FS_ANY, FS_ANY},
    {SPH_F_RHO,           FK_SCALAR, AT(h->rho),                                  S_ALL,   nullptr,                                                                    S_ALL,        0,      FS_ANY, FS_ANY},
    {SPH_F_PRESSURE,      FK_SCALAR, AT(wcsph_pressure(h)),                       SW,      "pressure is a wcsph field",                                                S_ALL & ~SD,  0,      FS_ANY, FS_ANY},
    {SPH_F_ALPHA,         FK_SCALAR, AT(dfsph_alpha(h)),                          SD,      "alpha is a dfsph field",                                                   SD,           0,      FS_ANY, FS_ANY},
    {SPH_F_WARM_K,        FK_SCALAR, AT(h->warm[h->wcur]),                        SD,      "warm_start_k is a dfsph field",                                            SD,           SD,     FS_ANY, FS_ANY},
    {SPH_F_RHO_ADV,       FK_SCALAR, AT(h->rho_adv),                              S_ALL,   nullptr,                                                                    S_ALL,        0,      FS_ANY, FS_ANY},
    {SPH_F_RHO_DER,       FK_SCALAR, AT(h->drho),                                 S_ALL,   nullptr,                                                                    S_ALL,        0,      FS_ANY, FS_ANY},
    {SPH_F_VEL_ADV,       FK_XYZ,    AT(h->VA[0]),                                SD | SI, "vel_adv is a dfsph / iisph field",                                         SD,           0,      FS_ANY, FS_ANY},
    {SPH_F_NBR_COUNT,     FK_COUNT,  AT(h->cnt),                                  S_ALL,   nullptr,                                                                    0,            0,      FS_ANY, FS_ANY},      // (a binned body: ncount, FK_INT)
    {SPH_F_PRESS_ITER,    FK_W,      AT(pci_fields(h).press[h->pb_final]),        SP | SI, "press_iter / p_iter is a pcisph / iisph field",                            0,            0,      FS_ANY, FS_ANY},
    {SPH_F_PRESS_FORCE,   FK_XYZ,    AT(h->cfg.solver == SPH_SOLVER_PCISPH ? pci_fields(h).press_force : ii_fields(h).f_press),
                                                                                  SP | SI, "press_force / f_press is a pcisph / iisph field",                          0,            0,      FS_ANY, FS_ANY},
    {SPH_F_POS_PREDICT,   FK_XYZ,    AT(h->cfg.solver == SPH_SOLVER_PBF ? h->P[h->pcur] : pci_fields(h).pos_predict),      // pbf: pos = pos_predict after a step (:84)
                                                                                  SP | SB, "pos_predict is a pcisph / pbf field",                                      SB,           0,      FS_ANY, FS_PBF_IN_ORDER},
    {SPH_F_D_II,          FK_XYZ,    AT(ii_fields(h).d_ii),                       SI,      "d_ii / d_ij are iisph fields",                                             0,            0,      FS_ANY, FS_ANY},
    {SPH_F_A_II,          FK_SCALAR, AT(ii_fields(h).a_ii),                       SI,      "a_ii is an iisph field",                                                   0,            0,      FS_ANY, FS_ANY},
    {SPH_F_D_IJ,          FK_XYZ,    AT(ii_fields(h).d_ij),                       SI,      "d_ii / d_ij are iisph fields",                                             0,            0,      FS_ANY, FS_ANY},
    {SPH_F_PBF_LAMBDA,    FK_SCALAR, AT(pbf_arrays(h).lambda),                    SB,      "pbf_lambda / delta_pos are pbf fields",                                    SB,           0,      FS_STEPPED, FS_PBF_IN_ORDER},
    {SPH_F_PBF_DELTA_POS, FK_XYZ,    AT(pbf_arrays(h).delta_pos),                 SB,      "pbf_lambda / delta_pos are pbf fields",                                    SB,           0,      FS_STEPPED, FS_PBF_IN_ORDER},
};
#undef AT

inline const FieldRow *fluid_field(int field)
{
    for (const FieldRow &r : kFluidFields) if (r.field == field) return &r;
    return nullptr;
}

struct FieldLoc { const void *data; FieldKind kind; };

// Where a fluid field of this handle is now, or why this view of it is refused.  FV_API: a field the table does not hold is the caller's to refuse
// (field_floats, before any size check)
int locate_field(SphHandle *h, int field, FieldView view, FieldLoc *out)
{
    const FieldRow *r = fluid_field(field);
    const unsigned solver = 1u << h->cfg.solver;
    if (view == FV_LOCAL) {
        if (!r || !(r->local & solver)) return fail(h, SPH_E_INVALID, "field %d cannot be downloaded from this handle", field);
        if (r->local_state == FS_PBF_IN_ORDER && !h->pbf_fields)
            return fail(h, SPH_E_STATE, h->simulate_cnt == 0 ? "pbf_lambda / delta_pos / pos_predict exist after the first step"
                                                             : "pbf_lambda / delta_pos / pos_predict of a slab handle are valid from a step until the next sort "
                                                               "(sph_build_neighbors, sph_compute_density, sph_slab_set_state): step first");
    } else {
        if (!r) return fail(h, SPH_E_INVALID, "field %d cannot be downloaded", field);
        if (!(r->owners & solver)) return fail(h, SPH_E_STATE, "%s", r->not_owner);
        if (r->api_state == FS_STEPPED && h->simulate_cnt == 0) return fail(h, SPH_E_STATE, "pbf_lambda / delta_pos exist after the first step");
    }
    *out = {r->at(h), r->kind};
    if (field == SPH_F_NBR_COUNT && rigid_binned(h)) *out = {h->ncount, FK_INT};      // get_neighbour_count with its rigid entries (ParticleSystem.py:436-444)
    return SPH_OK;
}

// a located field of the N particles of a one-GPU handle, in API order, as floats at `dst` (device)
void launch_unsort(SphHandle *h, const FieldLoc &f, float *dst)
{
    const dim3 g = grid_for(h->N), b(kBlock);
    hipStream_t s = h->stream;
    const int *id = h->id[h->icur];
    switch (f.kind) {
    case FK_XYZ: hipLaunchKernelGGL(k_unsort_vec, g, b, 0, s, h->N, (const float4 *)f.data, id, dst); break;
    case FK_SCALAR: hipLaunchKernelGGL(k_unsort_scalar, g, b, 0, s, h->N, (const float *)f.data, id, dst); break;
    case FK_W: hipLaunchKernelGGL(k_unsort_w, g, b, 0, s, h->N, (const float4 *)f.data, id, dst); break;
    case FK_COUNT: hipLaunchKernelGGL(k_unsort_count, g, b, 0, s, h->N, (const int *)f.data, id, dst); break;
    case FK_INT: hipLaunchKernelGGL(k_unsort_scalar_int, g, b, 0, s, h->N, (const int *)f.data, id, dst); break;
    }
}
// A per-particle array back in API order: `unsort` launches the caller's own kernel -- launch_unsort for an array of
// FieldLoc's kinds, k_unsort_planes for planes with a stride, an int or a measured-set kernel -- from device order through id[icur] into the staging
// area the caller names, under K_TRANSFER; then the check, `bytes` of it to the host, the wait.  The refusals (null pointer, element count) stay
// with the callers, in their own words and order.  (The device order does not change inside a step: the ids of the current generation apply)
template <class Unsort>
int fetch_api_order(SphHandle *h, Unsort unsort, const void *staging, void *host, size_t bytes)
{
    hipStream_t s = h->stream;
    {
        ProfScope ps(h, K_TRANSFER);
        unsort();
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(host, staging, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return SPH_OK;
}
// ... and back: floats in API order at `src` (device) into a float4 array's xyz or a float array
void launch_sort_in(SphHandle *h, const float *src, const FieldLoc &f)
{
    const dim3 g = grid_for(h->N), b(kBlock);
    if (f.kind == FK_XYZ) hipLaunchKernelGGL(k_sort_in_vec, g, b, 0, h->stream, h->N, src, h->id[h->icur], (float4 *)const_cast<void *>(f.data));
    else hipLaunchKernelGGL(k_sort_in_scalar, g, b, 0, h->stream, h->N, src, h->id[h->icur], (float *)const_cast<void *>(f.data));
}

// floats of a field as the API sizes it (N fluid particles, whatever is resident): every species
int field_floats(SphHandle *h, int species, int field, size_t *count)
{
    if (species == SPH_SPECIES_FLUID) {
        if (const FieldRow *r = fluid_field(field)) { *count = (r->kind == FK_XYZ ? 3 : 1) * (size_t)h->N; return SPH_OK; }
    } else if (species == SPH_SPECIES_WALL) {
        if (field == SPH_F_WALL_POS) { *count = 3 * (size_t)h->Nb; return SPH_OK; }
        if (field == SPH_F_WALL_VOL) { *count = (size_t)h->Nb; return SPH_OK; }
    } else if (species == SPH_SPECIES_RIGID && h->rigid) {
        if (field == SPH_F_RIGID_POS || field == SPH_F_RIGID_FORCE) { *count = 3 * (size_t)h->Nr; return SPH_OK; }
        if (field == SPH_F_RIGID_VOL || field == SPH_F_RIGID_MASS) { *count = (size_t)h->Nr; return SPH_OK; }
        if (field == SPH_F_RIGID_VERT) { *count = 3 * (size_t)h->Nv; return SPH_OK; }
    }
    return fail(h, SPH_E_INVALID, "unknown species/field %d/%d", species, field);
}
