// sph_host_wall_load.h -- a SECTION of csrc/sph_mi355x.hip's one translation unit (included there once, inside its anonymous namespace, in file order):
// the host side of the loads on walls and geometry (kernels in sph_wall_load_kernels.h).  Not a stand-alone header: it uses
// SphHandle and the helpers defined above its include.
//
// The measured set is built here, at selection time and at every edit of the wall set: the samples of the selected groups in the wall set's sorted
// order, their lists and totals, in one allocation of the feature's own.  A step of a handle with a selection launches, beside its own launches:
// k_wl_zero at its head, k_build_rnl on the set where the body's is launched, k_rigid_force / k_rigid_force_p<MODE> on the set at the solver's
// event, and the reduction pair at its end.  A handle without a selection launches none of them.

inline bool wl_on(const SphHandle *h) { return !h->wl_groups.empty(); }

inline WlView wl_view(const SphHandle *h)
{
    const SphHandle::WlMem &m = h->wl;
    return WlView{m.nm, (int)h->wl_groups.size(), m.MP, m.force, m.perm, m.seg};
}

// The measured set of the groups `ids` (selection order; every id is 0 or a group of `geo`) over the wall set `sorted` / `order` of Nb samples, into
// fresh memory: the lists zeroed (walk_list fetches past a row's end and relies on stale entries being valid indices), the totals zeroed, the
// accumulators zero or -- carry -- those the handle's present selection holds for the same id.  Nothing of the handle changes.  The handle's stream
// is idle (the callers have waited)
int wl_prepare(SphHandle *h, const char *call, const std::vector<int> &ids, const std::vector<float4> &sorted, const std::vector<int> &order, int Nb,
               const std::vector<SphHandle::GeoGroup> &geo, bool carry, SphHandle::WlMem *out, std::vector<SphHandle::WlGroup> *out_groups)
{
    std::vector<SphHandle::WlGroup> &groups = *out_groups;
    const int ng = (int)ids.size();
    int box = Nb;
    for (const auto &g : geo) box -= g.count;
    groups.clear();
    for (int id : ids) {
        int first = id == 0 ? 0 : box, count = id == 0 ? box : 0;
        for (size_t k = 0; id != 0 && k < geo.size(); ++k) {
            if (geo[k].id == id) { count = geo[k].count; break; }
            first += geo[k].count;
        }
        if (count <= 0) return fail(h, SPH_E_INVALID, "%s: no live group %d", call, id);
        groups.push_back({id, first, count});
    }
    std::vector<int> row_slot((size_t)Nb, -1);
    for (int s = 0; s < ng; ++s) std::fill(row_slot.begin() + groups[(size_t)s].first, row_slot.begin() + groups[(size_t)s].first + groups[(size_t)s].count, s);
    std::vector<float4> mp;
    std::vector<int> slot, local, seg((size_t)ng + 1, 0);
    for (int e = 0; e < Nb; ++e) {
        const int row = order[(size_t)e], s = row_slot[(size_t)row];
        if (s < 0) continue;
        mp.push_back(sorted[(size_t)e]);
        slot.push_back(s);
        local.push_back(row - groups[(size_t)s].first);
        seg[(size_t)s + 1]++;
    }
    const int nm = (int)mp.size();
    for (int s = 0; s < ng; ++s) seg[(size_t)s + 1] += seg[(size_t)s];
    std::vector<int> perm((size_t)nm), fill(seg.begin(), seg.end() - 1), ident((size_t)nm);
    for (int e = 0; e < nm; ++e) { perm[(size_t)fill[(size_t)slot[(size_t)e]]++] = e; ident[(size_t)e] = e; }
    std::vector<double> acc((size_t)ng * kWlAcc, 0.0);
    if (carry && h->wl.mem && !h->wl_groups.empty()) {
        std::vector<double> old(h->wl_groups.size() * kWlAcc);
        HIP_TRY(h, hipMemcpy(old.data(), h->wl.acc, sizeof(double) * old.size(), hipMemcpyDeviceToHost));
        for (int s = 0; s < ng; ++s)
            for (size_t k = 0; k < h->wl_groups.size(); ++k)
                if (h->wl_groups[k].id == ids[(size_t)s]) std::copy(old.begin() + (long)(k * kWlAcc), old.begin() + (long)((k + 1) * kWlAcc), acc.begin() + (long)((size_t)s * kWlAcc));
    }
    // one allocation of the set's own, zeroed
    SphHandle::WlMem &m = *out;
    const size_t n = (size_t)nm;
    m.nl_bytes = sizeof(uint32_t) * (n + 64) * (size_t)h->c.kpitch;
    m.mem.want(&m.MP, n + 64); m.mem.want(&m.nl, (n + 64) * (size_t)h->c.kpitch);
    m.mem.want(&m.cnt, n); m.mem.want(&m.ident, n); m.mem.want(&m.slot, n); m.mem.want(&m.local, n); m.mem.want(&m.perm, n); m.mem.want(&m.seg, (size_t)ng + 1);
    m.mem.want(&m.force, 3 * n); m.mem.want(&m.out, 3 * n);
    m.mem.want(&m.part, (size_t)ng * kWlParts * kWlRow); m.mem.want(&m.load, (size_t)ng * kWlRow); m.mem.want(&m.acc, (size_t)ng * kWlAcc);
    hipStream_t s = h->stream;
    HIP_TRY(h, m.mem.commit(s));
    m.nm = nm;
    HIP_TRY(h, hipMemcpyAsync(m.MP, mp.data(), sizeof(float4) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(m.ident, ident.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(m.slot, slot.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(m.local, local.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(m.perm, perm.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(m.seg, seg.data(), sizeof(int) * ((size_t)ng + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(m.acc, acc.data(), sizeof(double) * acc.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return SPH_OK;
}

// the built set becomes the handle's (no HIP call that can fail).  The captured wcsph step pairs hold or lack the feature's nodes and the old
// set's pointers: dropped, as sph_diag_record does
void wl_adopt(SphHandle *h, SphHandle::WlMem *m, std::vector<SphHandle::WlGroup> *groups)
{
    h->wl = std::move(*m);
    h->wl_groups.swap(*groups);
    mark_stale(h, STALE_LAUNCH_ARGS);
}

// ---- the launches of a step (all enqueued like any launch: no host wait, nodes of a captured wcsph step pair) ---------------------------------
void wl_step_head(SphHandle *h)
{
    ProfScope ps(h, K_WALL_LOAD);
    hipLaunchKernelGGL(k_wl_zero, grid_for(3 * h->wl.nm), dim3(kBlock), 0, h->stream, 3 * h->wl.nm, h->wl.force);
}

// the samples' view of the fluid, for the force launches of this step: k_build_rnl's rule, its "own cell" test included
void wl_build_lists(SphHandle *h)
{
    ProfScope ps(h, K_WALL_LOAD);
    hipLaunchKernelGGL(k_build_rnl, grid_for(h->wl.nm), dim3(kBlock), 0, h->stream, h->c, h->wl.nm, (const float4 *)h->wl.MP, (const float4 *)h->P[h->pcur],
                       (const int *)h->cell_start, h->wl.nl, h->wl.cnt, h->ds);
}

// wcsph / pcisph / iisph: launch_rigid_force_p on the measured set (a slab handle refuses the selection: no column window)
template <int MODE>
void wl_force_p(SphHandle *h, const float4 *P, const float4 *PB, int gate)
{
    ProfScope ps(h, K_WALL_LOAD);
    hipLaunchKernelGGL(k_rigid_force_p<MODE>, grid_for(h->wl.nm), dim3(kBlock), 0, h->stream, h->c, h->wl.nm, (const float4 *)h->wl.MP, (const int *)h->wl.ident, P,
                       (const uint32_t *)h->wl.nl, (const int *)h->wl.cnt, (const float *)h->rho, (const float *)wcsph_pressure(h), PB, (const DevScalars *)h->ds,
                       h->wl.force, gate, 0, 0, 0);
}

// dfsph: launch_rigid_force on the measured set, once per executed density iteration under the same gate
void wl_force_dfsph(SphHandle *h, int gate)
{
    ProfScope ps(h, K_WALL_LOAD);
    hipLaunchKernelGGL(k_rigid_force, grid_for(h->wl.nm), dim3(kBlock), 0, h->stream, h->c, h->wl.nm, (const float4 *)h->wl.MP, (const int *)h->wl.ident,
                       (const float4 *)h->P[h->pcur], (const uint32_t *)h->wl.nl, (const int *)h->wl.cnt, (const float *)h->rho, (const float *)h->rho_adv,
                       (const float *)dfsph_alpha(h), (const DevScalars *)h->ds, h->wl.force, gate, -0x7fffffff, 0x7fffffff);
}

// the reduction pair: about the point c into wl.load; accumulate (the end of a step, c = the origin): impulses and seconds go on
void wl_reduce(SphHandle *h, const double c[3], bool accumulate)
{
    const int ng = (int)h->wl_groups.size();
    int most = 1;
    for (const auto &g : h->wl_groups) most = std::max(most, g.count);
    const unsigned parts = (unsigned)std::min(kWlParts, (most + kBlock - 1) / kBlock);
    const bool device_dt = h->cfg.solver == SPH_SOLVER_DFSPH || h->step_adaptive;
    const WlView v = wl_view(h);
    hipLaunchKernelGGL(k_wl_partials, dim3(parts, (unsigned)ng), dim3(kBlock), 0, h->stream, v, c[0], c[1], c[2], h->wl.part);
    hipLaunchKernelGGL(k_wl_final, dim3((unsigned)ng), dim3(kBlock), 0, h->stream, v, StepDt{h->dt_wcsph, device_dt ? h->ds : nullptr}, (const double *)h->wl.part,
                       h->wl.load, accumulate ? h->wl.acc : (double *)nullptr);
}

void wl_step_end(SphHandle *h)
{
    ProfScope ps(h, K_WALL_LOAD);
    const double origin[3] = {0.0, 0.0, 0.0};
    wl_reduce(h, origin, true);
}

// fluid_count_changed: with fewer particles a stale entry of a measured list may name a particle that is gone
int wl_count_changed(SphHandle *h)
{
    if (!h->wl.mem) return SPH_OK;
    HIP_TRY(h, hipMemsetAsync(h->wl.nl, 0, h->wl.nl_bytes, h->stream));
    return SPH_OK;
}

// ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
int wl_refused(SphHandle *h, const char *call)
{
    if (h->slab) return fail(h, SPH_E_STATE, "%s is not available on a slab handle (a sample's fluid neighbours live on several ranks)", call);
    if (h->relaxed) return fail(h, SPH_E_STATE, "%s is not available under the relaxed arithmetic (its sweeps do not keep every operand of the force kernels)", call);
    if (h->cfg.solver == SPH_SOLVER_PBF) return fail(h, SPH_E_STATE, "%s: pbf moves positions and applies no forces", call);
    if (!h->c.boundary_handle) return fail(h, SPH_E_INVALID, "%s: the handle has clamp walls (boundary_handle 0): there are no wall samples", call);
    return SPH_OK;
}

int wall_load_select(SphHandle *h, const int32_t *groups, size_t n)
{
    if (int rc = wl_refused(h, "sph_wall_load_select")) return rc;
    if (n == 0) {                        // off: the memory stays (nothing a step reads is freed), the steps launch what they launched without it
        h->wl_groups.clear();
        mark_stale(h, STALE_LAUNCH_ARGS);
        return SPH_OK;
    }
    if (!groups) return fail(h, SPH_E_INVALID, "sph_wall_load_select: null groups");
    if (n > (size_t)kWlMaxGroups) return fail(h, SPH_E_INVALID, "sph_wall_load_select: %zu groups (at most %d)", n, kWlMaxGroups);
    std::vector<int> ids(groups, groups + n);
    for (size_t a = 0; a < n; ++a) {
        bool live = ids[a] == 0;
        for (const auto &g : h->geo_groups) live = live || g.id == ids[a];
        if (!live) return fail(h, SPH_E_INVALID, "sph_wall_load_select: no live group %d", ids[a]);
        for (size_t b = 0; b < a; ++b)
            if (ids[b] == ids[a]) return fail(h, SPH_E_INVALID, "sph_wall_load_select: group %d is named twice", ids[a]);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const int Nb = h->Nb;
    const std::vector<int> &order = h->wall_order_host;      // wall_tables' own, kept by build_scene and geometry_commit
    std::vector<float4> sorted((size_t)Nb);
    for (int e = 0; e < Nb; ++e) {
        const size_t j = (size_t)order[(size_t)e];
        sorted[(size_t)e] = make_float4(h->wall_pos_host[3 * j], h->wall_pos_host[3 * j + 1], h->wall_pos_host[3 * j + 2], h->wall_vol_host[j]);
    }
    SphHandle::WlMem next;                  // (built but not yet the handle's: freed unless adopted)
    std::vector<SphHandle::WlGroup> next_groups;
    if (int rc = wl_prepare(h, "sph_wall_load_select", ids, sorted, order, Nb, h->geo_groups, false, &next, &next_groups)) return rc;
    wl_adopt(h, &next, &next_groups);
    return SPH_OK;
}

// the place of `group` in the selection, -1 for "all selected" (*all), or the refusal
int wl_find(SphHandle *h, const char *call, int32_t group, int *slot, bool all_allowed)
{
    if (int rc = wl_refused(h, call)) return rc;
    if (!wl_on(h)) return fail(h, SPH_E_STATE, "%s: no wall group is selected (sph_wall_load_select)", call);
    *slot = -1;
    if (group == -1 && all_allowed) return SPH_OK;
    for (size_t k = 0; k < h->wl_groups.size(); ++k)
        if (h->wl_groups[k].id == group) { *slot = (int)k; return SPH_OK; }
    return fail(h, SPH_E_INVALID, "%s: group %d is not selected", call, group);
}

int wall_load_get(SphHandle *h, int32_t group, const double about[3], double force[3], double torque[3])
{
    int slot;
    if (int rc = wl_find(h, "sph_wall_load_get", group, &slot, true)) return rc;
    if (!force || !torque) return fail(h, SPH_E_INVALID, "sph_wall_load_get: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    const double origin[3] = {0.0, 0.0, 0.0};
    wl_reduce(h, about ? about : origin, false);
    HIP_TRY(h, hipGetLastError());
    std::vector<double> load(h->wl_groups.size() * kWlRow);
    HIP_TRY(h, hipMemcpyAsync(load.data(), h->wl.load, sizeof(double) * load.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int a = 0; a < 3; ++a) force[a] = torque[a] = 0.0;
    for (size_t k = 0; k < h->wl_groups.size(); ++k)            // all selected: the groups' sums in selection order
        if (slot < 0 || (size_t)slot == k)
            for (int a = 0; a < 3; ++a) { force[a] += load[k * kWlRow + (size_t)a]; torque[a] += load[k * kWlRow + 3 + (size_t)a]; }
    return SPH_OK;
}

// The samples do not move, so the angular impulse about c follows from the one about the origin: sum dt (x - c) x f = L_0 - c x J
int wall_load_impulse(SphHandle *h, int32_t group, const double about[3], double impulse[3], double angular[3], double *seconds, int reset)
{
    int slot;
    if (int rc = wl_find(h, "sph_wall_load_impulse", group, &slot, true)) return rc;
    if (!impulse || !angular || !seconds) return fail(h, SPH_E_INVALID, "sph_wall_load_impulse: null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t ng = h->wl_groups.size();
    std::vector<double> acc(ng * kWlAcc);
    HIP_TRY(h, hipMemcpyAsync(acc.data(), h->wl.acc, sizeof(double) * acc.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    // "all selected" is one window: after a reset of a single group the groups have measured for different lengths of time, and a sum of their
    // impulses over one `seconds` would be no mean force of anything
    for (size_t k = 1; slot < 0 && k < ng; ++k)
        if (acc[k * kWlAcc + 6] != acc[6])
            return fail(h, SPH_E_STATE, "sph_wall_load_impulse: the selected groups have measured for different times (%g s and %g s, after a reset of one group): "
                                        "read them one by one, or reset them all", acc[6], acc[k * kWlAcc + 6]);
    double J[3] = {0, 0, 0}, L[3] = {0, 0, 0};
    for (size_t k = 0; k < ng; ++k)
        if (slot < 0 || (size_t)slot == k)
            for (int a = 0; a < 3; ++a) { J[a] += acc[k * kWlAcc + (size_t)a]; L[a] += acc[k * kWlAcc + 3 + (size_t)a]; }
    const double c[3] = {about ? about[0] : 0.0, about ? about[1] : 0.0, about ? about[2] : 0.0};
    for (int a = 0; a < 3; ++a) impulse[a] = J[a];
    angular[0] = L[0] - (c[1] * J[2] - c[2] * J[1]);
    angular[1] = L[1] - (c[2] * J[0] - c[0] * J[2]);
    angular[2] = L[2] - (c[0] * J[1] - c[1] * J[0]);
    *seconds = acc[(size_t)(slot < 0 ? 0 : slot) * kWlAcc + 6];
    if (reset) {
        if (slot < 0) HIP_TRY(h, hipMemsetAsync(h->wl.acc, 0, sizeof(double) * ng * kWlAcc, h->stream));
        else HIP_TRY(h, hipMemsetAsync(h->wl.acc + (size_t)slot * kWlAcc, 0, sizeof(double) * kWlAcc, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return SPH_OK;
}

int wall_load_forces(SphHandle *h, int32_t group, float *xyz, size_t n_floats)
{
    int slot;
    if (int rc = wl_find(h, "sph_wall_load_forces", group, &slot, false)) return rc;
    if (!xyz) return fail(h, SPH_E_INVALID, "sph_wall_load_forces: null argument");
    const size_t want = 3 * (size_t)h->wl_groups[(size_t)slot].count;
    if (n_floats != want) return fail(h, SPH_E_INVALID, "sph_wall_load_forces: group %d has %d samples, got room for %zu floats", group, h->wl_groups[(size_t)slot].count, n_floats);
    HIP_TRY(h, hipSetDevice(h->device));
    return fetch_api_order(h, [&] {
        hipLaunchKernelGGL(k_wl_unsort, grid_for(h->wl.nm), dim3(kBlock), 0, h->stream, h->wl.nm, slot, (const int *)h->wl.slot, (const int *)h->wl.local,
                           (const float *)h->wl.force, h->wl.out);
    }, h->wl.out, xyz, sizeof(float) * want);
}
