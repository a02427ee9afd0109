// sph_host_flow.h -- a section of sph_mi355x.hip's translation unit (included inside its anonymous namespace): what the calls that change a
// handle's particle count between steps share (sph_add_particles, sph_remove_in_box, sph_geometry_carve).
#pragma once

// ---- inlets and sinks ---------------------------------------------------------------------------------------
static int flow_refused(SphHandle *h, const char *call)
{
    if (h->slab) return fail(h, SPH_E_STATE, "%s is not available on a slab handle", call);
    if (h->rigid) return fail(h, SPH_E_STATE, "%s is not available on a handle with a rigid body", call);
    return SPH_OK;
}

// The live count is now `n`: what the host caches from it, and what the steps so far left behind that a fresh handle of these particles would
// not have (forget_step_history, as sph_slab_set_state) -- but for what travels with the handle: delta_time, the clock, gravity and forcing, the
// carried scalars of the particles that stay, pcisph's delta, last_iters and pb_final.
static int fluid_count_changed(SphHandle *h, int n)
{
    hipStream_t s = h->stream;
    h->N = n; h->n_owned = n;
    h->c.n = n;
    h->nblocks = (n + kBlock - 1) / kBlock;
    if (int rc = forget_step_history(h)) return rc;
    const void *tile_flags[] = {h->pci_zero_press};
    if (int rc = dzero(h, tile_flags, 1)) return rc;
    if (int rc = wl_count_changed(h)) return rc;                      // the measured wall samples' lists (section 6m): stale entries must stay valid indices
    // the lists of the last build know neither the new particles nor the new slots; the captured step pairs carry the old count and grids
    if (int rc = mark_stale(h, STALE_COUNT)) return rc;
    HIP_TRY(h, hipStreamSynchronize(s));
    // The run diagnostics (section 6i) need nothing here: their launches take the live count of the moment as an argument and keep no state about
    // particles -- a recording goes on, its next row counts the new n
    return SPH_OK;
}

// Remove every particle on which `gone` says 1 (RemoveBox, RemoveMarked: sph_kernels.h) and compact the survivors: id order kept, the carried
// scalar with them.  flags(n, P, id, flag_slot, flag_id) launches the kernel that writes the two flag arrays -- and whatever `gone` reads.
// `holds`: the subject of the refusal when nobody would be left
template <class Pred, class Flags>
int remove_where(SphHandle *h, const char *call, const char *holds, const Pred &gone, Flags flags, int32_t *removed)
{
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    HIP_TRY(h, hipStreamSynchronize(s));
    const int n = h->c.n, stride = h->c.stride, nt = (n + kScanTile - 1) / kScanTile;
    // scratch between steps: the sort's three int arrays (rewritten by the next sort before anything reads them) and the staging buffer as
    // three int arrays of `stride` entries -- the scan over ids, the two scans' tile sums, the count in the last word
    int *flag_slot = h->cell_of, *flag_id = h->rank, *scan_slot = h->slot_src;
    int *scan_id = (int *)h->staging, *sums_slot = scan_id + stride, *sums_id = scan_id + 2 * (size_t)stride, *total = scan_id + 3 * (size_t)stride - 1;
    const dim3 g = grid_for(n), b(kBlock);
    const float4 *P = h->P[h->pcur];
    const int *id = h->id[h->icur];
    {
        ProfScope ps(h, K_TRANSFER);
        flags(n, P, id, flag_slot, flag_id);
        hipLaunchKernelGGL(k_scan_tiles, dim3(nt), b, 0, s, flag_slot, scan_slot, sums_slot, n, (const int *)nullptr);
        hipLaunchKernelGGL(k_scan_sums, dim3(1), b, 0, s, sums_slot, nt, (const int *)nullptr);
        hipLaunchKernelGGL(k_scan_add, g, b, 0, s, scan_slot, (const int *)sums_slot, n, (const int *)nullptr, 0);
        hipLaunchKernelGGL(k_scan_tiles, dim3(nt), b, 0, s, flag_id, scan_id, sums_id, n, (const int *)nullptr);
        hipLaunchKernelGGL(k_scan_sums, dim3(1), b, 0, s, sums_id, nt, (const int *)nullptr);
        hipLaunchKernelGGL(k_scan_add, g, b, 0, s, scan_id, (const int *)sums_id, n, (const int *)nullptr, 0);
        hipLaunchKernelGGL((k_remove_count<Pred>), dim3(1), dim3(1), 0, s, n, gone, P, (const int *)scan_slot, total);
    }
    HIP_TRY(h, hipGetLastError());
    int r = -1;
    HIP_TRY(h, hipMemcpyAsync(&r, total, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (r < 0 || r > n) return fail(h, SPH_E_STATE, "internal: %s counted %d of %d particles", call, r, n);
    if (r == n) return fail(h, SPH_E_INVALID, "%s: %s all %d particles (an empty handle is not supported)", call, holds, n);
    if (removed) *removed = r;
    if (r == 0) return SPH_OK;
    const bool carry = carries_scalar(h);
    {
        ProfScope ps(h, K_TRANSFER);
        hipLaunchKernelGGL((k_remove_compact<Pred>), g, b, 0, s, n, gone, (const int *)scan_slot, (const int *)scan_id, P, (const float4 *)h->V[h->vcur],
                           carry ? (const float *)h->warm[h->wcur] : (const float *)nullptr, id, h->P[1 - h->pcur], h->V[1 - h->vcur], h->warm[1 - h->wcur],
                           h->id[1 - h->icur]);
    }
    HIP_TRY(h, hipGetLastError());
    if (scalar_on(h))
        if (int rc = scalar_compact(h, n, n - r, gone, P, id, scan_id)) return rc;
    h->pcur ^= 1; h->vcur ^= 1; h->icur ^= 1;
    if (carry) h->wcur ^= 1;
    return fluid_count_changed(h, n - r);
}
