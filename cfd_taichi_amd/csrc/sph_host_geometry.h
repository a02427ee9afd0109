// sph_host_geometry.h -- a section of sph_mi355x.hip's translation unit (included inside its anonymous namespace): the edits of a handle's wall
// set between steps.  Carving removes particles through remove_where (sph_host_flow.h).
#pragma once

// ---- static geometry ----------------------------------------------------------------------------------------
inline int geo_box_count(const SphHandle *h)
{
    int nb0 = h->Nb;
    for (const auto &g : h->geo_groups) nb0 -= g.count;
    return nb0;
}

// The wall set becomes `pos` (3 Nb floats: the box samples, then `groups` in order).  Everything is computed into temporaries first; a refusal
// leaves the handle as it was.  On success: the tables of wall_tables() on the device and in the host copies, and nothing of the last list build
// left standing that was derived from the old set.
static int geometry_commit(SphHandle *h, const char *call, std::vector<float> &pos, int Nb, std::vector<SphHandle::GeoGroup> &groups)
{
    const Consts &c = h->c;
    if ((long long)Nb >= (1LL << 28)) return fail(h, SPH_E_INVALID, "%s: %d wall samples (a handle addresses its wall array with 32-bit byte offsets: < 2^28)", call, Nb);
    std::vector<float> vol;
    std::vector<float4> sorted;
    std::vector<int> wcell_start, order;
    if (int rc = wall_tables(h, pos, Nb, vol, sorted, wcell_start, order)) return rc;
    for (int i = 0; i < Nb; ++i)
        if (!std::isfinite(vol[i]))
            return fail(h, SPH_E_INVALID, "%s: wall sample %d would have no other sample within h = %g (its kernel sum is zero, its volume infinite)", call, i, (double)c.h);
    // the group of every sample, in sorted order
    std::vector<int> group_of((size_t)Nb, 0), wgroup((size_t)Nb);
    {
        size_t at = (size_t)Nb;
        for (size_t k = groups.size(); k-- > 0;) {
            at -= (size_t)groups[k].count;
            std::fill(group_of.begin() + (long)at, group_of.begin() + (long)(at + (size_t)groups[k].count), groups[k].id);
        }
    }
    for (int e = 0; e < Nb; ++e) wgroup[(size_t)e] = group_of[(size_t)order[(size_t)e]];

    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    HIP_TRY(h, hipStreamSynchronize(s));
    if (h->xstream) HIP_TRY(h, hipStreamSynchronize(h->xstream));
    if (h->rstream) HIP_TRY(h, hipStreamSynchronize(h->rstream));
    // Loads on walls (section 6m): the selection is kept by id -- a removed group leaves it, the impulses of the others go on.  The measured set of
    // the new wall set is built here, into memory of its own, before anything of the handle changes (a refusal leaves the selection as it was) ...
    SphHandle::WlMem wl_next;
    std::vector<SphHandle::WlGroup> wl_next_groups;
    std::vector<int> wl_ids;
    for (const auto &sel : h->wl_groups)
        for (size_t k = 0; k <= groups.size(); ++k)
            if (k == groups.size() ? sel.id == 0 : groups[k].id == sel.id) { wl_ids.push_back(sel.id); break; }
    if (!wl_ids.empty())
        if (int rc = wl_prepare(h, call, wl_ids, sorted, order, Nb, groups, true, &wl_next, &wl_next_groups)) return rc;
    // The device copy never shrinks: the sweeps fetch a group of list entries past a row's end and rely on stale entries being valid indices
    // (walk_list, sph_kernels.h).  Memory of the feature's own; the arena's WP is simply no longer pointed to
    // Every edit uploads into a fresh allocation through local pointers; the handle's fields change only behind the final wait, so a HIP error on
    // the way leaves the handle as it was.  Edits are rare: an allocation per edit costs nothing that matters
    DevMem mem;
    const size_t cap = std::max(h->geo_cap, (size_t)Nb + (size_t)Nb / 2);
    float4 *wp_dev = nullptr;
    int *wgroup_dev = nullptr, *marked_dev = nullptr;
    mem.want(&wp_dev, cap + 64);
    mem.want(&wgroup_dev, cap + 64);
    mem.want(&marked_dev, (size_t)c.stride);
    HIP_TRY(h, mem.commit(s));
    hipError_t e = hipMemcpyAsync(wp_dev, sorted.data(), sizeof(float4) * (size_t)Nb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(wgroup_dev, wgroup.data(), sizeof(int) * (size_t)Nb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(h, SPH_E_HIP, "%s: upload of the wall tables: %s", call, hipGetErrorString(e));
    // from here on the handle changes: the cell starts (arena memory, read together with WP), the wall lists, the pointers
    HIP_TRY(h, hipMemcpyAsync(h->wcell_start, wcell_start.data(), sizeof(int) * ((size_t)c.C + 1), hipMemcpyHostToDevice, s));
    // ... and the wall lists are zeroed once, as the freeze zeroes the fluid lists (sph_rigid_set_active): index 0 is valid in every list format
    const void *lists[] = {h->nlb};
    if (int rc = dzero(h, lists, 1)) return rc;
    // what the last list build derived from the old wall set: the lists (Verlet ones included) and counts, the density, the derived fields; the
    // captured wcsph step pairs hold WP, wcell_start and the kernels' arguments of their capture.  The density loop's working-tiles-first order is a
    // launch order only; it starts afresh as on a new handle.  Fluid state, clock, dt, warm start, pcisph's delta, gravity, scalar, recording and
    // the body are not touched
    if (int rc = mark_stale(h, STALE_WALL_SET)) return rc;
    HIP_TRY(h, hipStreamSynchronize(s));
    h->own.geometry = std::move(mem); h->geo_cap = cap;
    h->WP = wp_dev; h->geo_wgroup = wgroup_dev; h->geo_marked = marked_dev;
    h->Nb = Nb;
    h->geo_groups.swap(groups);
    pos.resize(3 * (size_t)Nb);
    h->wall_pos_host.swap(pos);
    h->wall_vol_host.swap(vol);
    h->wall_order_host.swap(order);
    // ... and becomes the handle's here; the last step's forces read zero until a step has run.  Nobody left of the selection: measuring is off
    if (!wl_ids.empty()) wl_adopt(h, &wl_next, &wl_next_groups);
    else h->wl_groups.clear();
    return SPH_OK;
}

static int geometry_refused(SphHandle *h, const char *call)
{
    if (!h->c.boundary_handle) return fail(h, SPH_E_INVALID, "%s: the handle has clamp walls (boundary_handle 0): its sweeps never walk wall lists", call);
    return SPH_OK;
}

int geometry_add(SphHandle *h, const float *xyz, size_t n, int32_t *group)
{
    if (int rc = geometry_refused(h, "sph_geometry_add")) return rc;
    if (!xyz) return fail(h, SPH_E_INVALID, "sph_geometry_add: null positions");
    if (n == 0) return fail(h, SPH_E_INVALID, "sph_geometry_add: a group of no samples");
    if (n >= ((size_t)1 << 28) || (long long)h->Nb + (long long)n >= (1LL << 28))
        return fail(h, SPH_E_INVALID, "sph_geometry_add: %d + %zu wall samples (a handle addresses its wall array with 32-bit byte offsets: < 2^28)", h->Nb, n);
    const Consts &c = h->c;
    const int g3[3] = {c.gx, c.gy, c.gz};
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const float x = xyz[3 * i + a];
            if (!std::isfinite(x)) return fail(h, SPH_E_INVALID, "sph_geometry_add: sample %zu has a coordinate that is not finite", i);
            const float cell = floorf(x / c.hcell);
            if (!(cell >= 0.f && cell < (float)g3[a]))
                return fail(h, SPH_E_INVALID, "sph_geometry_add: sample %zu lies at %g on axis %d, outside the cell grid (%d cells of %g)", i, (double)x, a, g3[a], (double)c.hcell);
        }
    std::vector<float> pos(h->wall_pos_host.begin(), h->wall_pos_host.begin() + 3 * (long)h->Nb);
    pos.insert(pos.end(), xyz, xyz + 3 * n);
    std::vector<SphHandle::GeoGroup> groups = h->geo_groups;
    groups.push_back({h->geo_next_id, (int)n});
    if (int rc = geometry_commit(h, "sph_geometry_add", pos, h->Nb + (int)n, groups)) return rc;
    if (group) *group = h->geo_next_id;
    h->geo_next_id++;                                               // ids are never reused
    return SPH_OK;
}

int geometry_remove(SphHandle *h, int32_t group)
{
    if (int rc = geometry_refused(h, "sph_geometry_remove")) return rc;
    size_t k = 0, first = (size_t)geo_box_count(h);
    for (; k < h->geo_groups.size() && h->geo_groups[k].id != group; ++k) first += (size_t)h->geo_groups[k].count;
    if (k == h->geo_groups.size()) return fail(h, SPH_E_INVALID, "sph_geometry_remove: no live group %d", group);
    const size_t cnt = (size_t)h->geo_groups[k].count;
    // the gap closes: later groups move down and keep their ids
    std::vector<float> pos(h->wall_pos_host.begin(), h->wall_pos_host.begin() + 3 * (long)h->Nb);
    pos.erase(pos.begin() + 3 * (long)first, pos.begin() + 3 * (long)(first + cnt));
    std::vector<SphHandle::GeoGroup> groups = h->geo_groups;
    groups.erase(groups.begin() + (long)k);
    return geometry_commit(h, "sph_geometry_remove", pos, h->Nb - (int)cnt, groups);
}

int geometry_info(SphHandle *h, int32_t *groups, int32_t *first, int32_t *count, size_t cap, size_t *n_groups)
{
    if (!n_groups || (cap > 0 && (!groups || !first || !count))) return fail(h, SPH_E_INVALID, "sph_geometry_info: null argument");
    int at = geo_box_count(h);
    for (size_t k = 0; k < h->geo_groups.size(); ++k) {
        if (k < cap) { groups[k] = h->geo_groups[k].id; first[k] = at; count[k] = h->geo_groups[k].count; }
        at += h->geo_groups[k].count;
    }
    *n_groups = h->geo_groups.size();
    return SPH_OK;
}

int geometry_carve(SphHandle *h, int32_t group, float clearance, int32_t *removed)
{
    if (int rc = geometry_refused(h, "sph_geometry_carve")) return rc;
    if (int rc = flow_refused(h, "sph_geometry_carve")) return rc;
    if (!(clearance > 0.f && clearance <= h->c.h)) return fail(h, SPH_E_INVALID, "sph_geometry_carve: clearance %g outside (0, h = %g]", (double)clearance, (double)h->c.h);
    bool live = group == -1;
    for (const auto &g : h->geo_groups) live = live || g.id == group;
    if (!live) return fail(h, SPH_E_INVALID, "sph_geometry_carve: no live group %d", group);
    if (h->geo_groups.empty()) { if (removed) *removed = 0; return SPH_OK; }      // every added group, and there is none
    const RemoveMarked gone = {h->geo_marked};
    return remove_where(h, "sph_geometry_carve", "the clearance takes", gone, [&](int n, const float4 *P, const int *id, int *flag_slot, int *flag_id) {
        hipLaunchKernelGGL(k_carve_flag, grid_for(n), dim3(kBlock), 0, h->stream, h->c, (int)group, clearance, P, id, (const float4 *)h->WP,
                           (const int *)h->wcell_start, (const int *)h->geo_wgroup, flag_slot, flag_id, h->geo_marked);
    }, removed);
}

// The wall entries of every particle's list as the last list build left them, in API order (through the staging buffer as ints)
int geometry_wall_counts(SphHandle *h, int32_t *counts, size_t n)
{
    if (h->slab) return fail(h, SPH_E_STATE, "sph_geometry_wall_counts is not available on a slab handle");
    if (!counts) return fail(h, SPH_E_INVALID, "sph_geometry_wall_counts: null argument");
    if (n != (size_t)h->N) return fail(h, SPH_E_INVALID, "sph_geometry_wall_counts: the handle holds %d particles, got room for %zu", h->N, n);
    HIP_TRY(h, hipSetDevice(h->device));
    return fetch_api_order(h, [&] {
        hipLaunchKernelGGL(k_unsort_wall_count, grid_for(h->N), dim3(kBlock), 0, h->stream, h->N, (const int *)h->cnt, (const int *)h->id[h->icur], (int *)h->staging);
    }, h->staging, counts, sizeof(int32_t) * n);
}
