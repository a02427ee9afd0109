"""What the slab test workers share: `world` ranks on ONE GPU, their owned particles gathered by id and compared bit for bit with a one-GPU handle.

Two ways to get the ranks.  The loopback group (Ranks): `world` slab handles of one process on the library's NATIVE transport (ncclSend / ncclRecv /
ncclAllReduce issued by the library itself on its main, halo and reduction streams), with tests/loopback_rccl.hip standing in for librccl
(SPH_RCCL_LIB, a development override: loopback_env) and moving the bytes device-to-device under the same ordering rules.  A collective call must
run on every rank at once, one thread each: Ranks.each.  Or one process per rank under torch.distributed.run, SlabSimulation over the callback
transport: process_group.

Plain Python: no torch and no library at module level (the workers hand in `nat` = cfd_taichi_amd._native), so this imports anywhere."""
import contextlib
import hashlib
import json
import os
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shim_path(build=True):
    so = os.path.join(ROOT, "tests", "_build", "libloopback_rccl.so")
    src = os.path.join(ROOT, "tests", "loopback_rccl.hip")
    if build and (not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src)):
        import subprocess
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", src, "-o", so], check=True, cwd=ROOT)
    return so


def loopback_env():
    """before the library loads: the stand-in as a named development override, the slabs' self-checks on unless the caller chose"""
    os.environ["SPH_DEV"] = "1"
    os.environ["SPH_RCCL_LIB"] = shim_path()
    os.environ.setdefault("SPH_SLAB_CHECK", "1")


def stat_row(st):
    return None if st is None else [st.n_div, st.n_dens, st.n_div_evals, float(st.div_first_err), float(st.div_err), float(st.dens_err), float(st.dt)]


def gather_by_id(sims, field):
    """(out, seen): the handles' owned particles in original order (NaN where nobody owns one), and how many handles own each id -- all 1 for a partition"""
    n = sims[0].n_fluid
    out, seen = None, np.zeros(n, dtype=np.int32)
    for s in sims:
        ids, vals = s.download_owned(field)
        if out is None:
            out = np.full((n,) + vals.shape[1:], np.nan, dtype=np.float32)
        out[ids] = vals
        np.add.at(seen, ids, 1)
    return out, seen


def owned_samples(sample_x, h, cols):
    """how many of a body's samples lie in a slab's owned cell columns [x_lo, x_hi), from the samples' x and the cell edge (both f32)"""
    col = np.floor(sample_x / h).astype(np.int64)
    return int(((col >= cols[0]) & (col < cols[1])).sum())


class Ranks:
    """`world` slab handles of one process on the loopback transport, attached.  per_rank: {rank: config_from_dict keywords of that rank alone}."""

    def __init__(self, nat, cfg, world, rigid=None, per_rank=None, **config_opts):
        self.nat, self.world = nat, world
        self.active = bool(rigid and rigid.get("active"))
        self.wcsph = nat.config_from_dict(cfg).solver == nat.SOLVER_WCSPH
        self.errors = [None] * world
        self.sims = [nat.Simulation(nat.config_from_dict(cfg, slab_rank=r, slab_count=world, **dict(config_opts, **(per_rank or {}).get(r, {}))), rigid=rigid)
                     for r in range(world)]
        uid = nat.rccl_unique_id()
        self.each(lambda r, s: s.rccl_attach(uid, 64 << 20))              # collective: returns when every rank has joined

    def each(self, fn):
        """fn(rank, sim) on every rank at once; returns the results, raises the first exception after ALL threads have ended (.errors keeps every rank's)"""
        out, err = [None] * self.world, [None] * self.world

        def run(r):
            try:
                out[r] = fn(r, self.sims[r])
            except BaseException as e:  # noqa: BLE001 - reported below; the other ranks run into the stand-in's bounded waits
                err[r] = e
        threads = [threading.Thread(target=run, args=(r,)) for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        self.errors = err
        for e in err:
            if e is not None:
                raise e
        return out

    def codes(self, fn):
        """the SphError code of fn on every rank (0: no error)"""
        try:
            self.each(fn)
        except self.nat.SphError:
            pass
        return [0 if e is None else getattr(e, "code", repr(e)) for e in self.errors]

    def step(self):
        """one step on every rank (any solver but wcsph: and the body step after it when the body is active); every rank's stat_row"""
        def one(r, s):
            if self.wcsph:
                s.step_wcsph(1)
                return None
            st = stat_row(s.step(1))
            if self.active:
                s.rigid_step()
            return st
        return self.each(one)

    def gather(self, field):
        out, seen = gather_by_id(self.sims, field)
        assert np.all(seen == 1), "slab ownership is not a partition: %d missing, %d duplicated" % (int((seen == 0).sum()), int((seen > 1).sum()))
        return out

    def owners(self):
        own = np.full(self.sims[0].n_fluid, -1, dtype=np.int32)
        for r, s in enumerate(self.sims):
            own[s.download_owned(self.nat.F_POS)[0]] = r
        return own

    def infos(self):
        return [s.slab_info() for s in self.sims]

    def cuts(self):
        infos = self.infos()
        return [i["x_lo"] for i in infos] + [infos[-1]["x_hi"]]

    def digest(self):
        """everything resident on every rank, ghosts included, by particle id"""
        h = hashlib.sha1()
        for s in self.sims:
            for field in (self.nat.F_POS, self.nat.F_VEL, self.nat.F_RHO):
                ids, vals = s.download_local(field)
                order = np.argsort(ids, kind="stable")
                h.update(ids[order].tobytes()); h.update(vals[order].tobytes())
            h.update(json.dumps(s.slab_info(), sort_keys=True).encode())
        return h.hexdigest()

    def close(self):
        for s in self.sims:
            s.close()


@contextlib.contextmanager
def process_group(backend="gloo"):
    """(rank, world, device) of a worker under torch.distributed.run; on the way out the closing barrier and the group's end"""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    device = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    if backend == "nccl":
        torch.cuda.set_device(device)
        dist.init_process_group("nccl", device_id=torch.device("cuda", device))
    else:
        dist.init_process_group(backend)
    yield rank, world, device
    dist.barrier()
    dist.destroy_process_group()


def body_ranks(args, cfg, rigid, per_rank, compare):
    """A body on slab handles over args.transport (gloo: SlabSimulation + TorchComm, one process per rank; loopback: args.world handles, one thread
    per rank around its whole run), args.rebalance steps between re-cuts.  per_rank(nat, native, full_step) -> that rank's report, native its
    nat.Simulation and full_step() one solver step and the body step after it.  Rank 0 (loopback: the process) writes what
    compare(nat, reports, [pos, vel, rho] gathered by id) returns to args.out, on the loopback with every handle's overrides."""
    def write(result):
        with open(args.out, "w") as f:
            json.dump(result, f)
    if args.transport == "gloo":
        import torch.distributed as dist
        with process_group() as (rank, world, device):
            from cfd_taichi_amd import _native as nat
            from cfd_taichi_amd.slab import SlabSimulation
            sim = SlabSimulation(cfg, rank, world, device=device, rebalance_every=args.rebalance)
            rep = per_rank(nat, sim.sim, lambda: sim.step(1))
            reps = [None] * world if rank == 0 else None
            dist.gather_object(rep, reps, dst=0)
            fields = [sim.gather(f) for f in (nat.F_POS, nat.F_VEL, nat.F_RHO)]
            if rank == 0:
                write(compare(nat, reps, fields))
            sim.close()
        return
    loopback_env()
    from cfd_taichi_amd import _native as nat
    g = Ranks(nat, cfg, args.world, rigid=rigid, slab_rebalance_every=args.rebalance)

    def run(r, s):
        def full_step():
            st = s.step(1)
            s.rigid_step()
            return st
        return per_rank(nat, s, full_step)
    reps = g.each(run)
    result = compare(nat, reps, [g.gather(f) for f in (nat.F_POS, nat.F_VEL, nat.F_RHO)])
    write(dict(result, overrides=[s.overrides() for s in g.sims]))
    g.close()
