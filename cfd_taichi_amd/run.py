"""Headless runner: the reference's frame loop (main.py:95-206) without the GGUI window.

    python -m cfd_taichi_amd.run --config config/dfsph_small.json [--solver dfsph] [--until 4.0 | --steps N] [--ply-dir output]
    torchrun --nproc-per-node 8 -m cfd_taichi_amd.run --config config/dfsph_10m.json --steps 100      # one x-slab per GPU (no rigid body)

Per frame: `iter_cnt` fluid steps, then `iter_cnt` rigid steps if a rigid body is active (main.py:165-171),
t += iter_cnt * solver.delta_time[None] (:173); stops at t > 4.0 (:205) or after --steps frames.  With --ply-dir (or
scene.is_output_ply) it writes ASCII PLY frames `output_%06d.ply` at scene.output_fps like main.py:189-195 (vertex
xyz + the constant RGBA of ParticleSystem.py:152) and, when a rigid body exists, `obj_%06d.obj` of its mesh (:196-200).
--release-rigid-at FRAME runs the release sequence the reference keeps commented out at main.py:100-106 when frame_cnt reaches FRAME: a body
created with `solid.active: false` drops into the fluid as it is then.
`scene.emitters` / `scene.sinks` (cfd_taichi_amd/emitter.py; the handle needs a `fluid.capacity`): after every solver step the sinks are applied,
then the emitters; the PLY frames hold the particles of the moment.  Single GPU, no rigid body.
--diag-csv PATH [--diag-every N]: the fluid's run diagnostics (energy, momentum, centre of mass, extent, ...; _native.DIAG_SLOTS), summed on the device at
the end of every N-th solver step and drained once per frame; one CSV line per recorded step under a header of the slot names, written at the end of
the run.  Single GPU.
--ply-fields vorticity,divergence,normal,cover: derived per-particle fields (Simulation.derived) as further `property float` columns of every PLY
frame, after alpha: vort_x vort_y vort_z div normal_x normal_y normal_z cover -- only the named ones, always in that order.  `scalar`: the carried
scalar (scene.scalar; Simulation.scalar()) as one more column `scalar` behind them.  Single GPU.
`scene.geometry` (cfd_taichi_amd/geometry.py): static obstacles as wall samples, applied when the handle is made.
--remove-geometry NAME@FRAME (repeatable) takes the entry NAME out of the wall set when frame_cnt reaches FRAME: pulls a gate; sharded runs too.
--geometry-ply DIR writes the wall samples, box and geometry, with an int `group` column as `geometry_%06d.ply` at frame 0 and after every edit.
Single GPU.  While loads are measured the file carries three more float columns fx fy fz: the last step's force on every sample of a measured group,
zero elsewhere.
`scene.loads` (["box", "gate", ...]): the wall groups whose load is measured on the device while the steps run; skipped
with one printed line where loads cannot be measured (sharded runs, --arith relaxed, pbf).
--load-csv PATH: one line per frame and measured group -- frame, time, group, the seconds the frame covered, the mean force and the mean torque
about the origin over the frame (impulse / seconds), and the last step's force -- written at the end of the run.  Single GPU.
Without the flags a run does what it did."""
import argparse
import importlib
import os
import time

import numpy as np

from . import ParticleSystem, emitter, rigid_solver, utils


LAST = {}      # the objects of the last single-GPU main() call (ps, solver, rigid), for a caller that embeds the runner and reads the end state


# --ply-fields: the derived fields a PLY frame can carry, in column order, with their column names
PLY_FIELDS = (("vorticity", ("vort_x", "vort_y", "vort_z")), ("divergence", ("div",)), ("normal", ("normal_x", "normal_y", "normal_z")), ("cover", ("cover",)))
PLY_SCALAR = "scalar"          # ... and the carried scalar, which is no derived field: always the last column


def parse_ply_fields(text):
    """the names of --ply-fields in column order (whatever order they were given in); an unknown name ends the run"""
    asked = [w.strip() for w in (text or "").split(",") if w.strip()]
    known = [name for name, _ in PLY_FIELDS] + [PLY_SCALAR]
    for w in asked:
        if w not in known:
            raise SystemExit("--ply-fields: unknown field '%s' (choose from %s)" % (w, ", ".join(known)))
    return [name for name in known if name in asked]


def ply_extra(sim, fields):
    """[(column names, (n, k) values)] of the named derived fields of the state `sim` holds, the carried scalar behind them"""
    cols = dict(PLY_FIELDS)
    out = [(cols[name], sim.derived(name).reshape(sim.n_fluid, -1)) for name in fields if name != PLY_SCALAR]
    if PLY_SCALAR in fields:
        out.append(((PLY_SCALAR,), sim.scalar().reshape(sim.n_fluid, 1)))
    return out


def write_ply_ascii(path, pos, rgba, extra=()):
    """ASCII PLY in the layout of ti.tools.PLYWriter.export_frame_ascii: float x y z red green blue alpha; extra: [(column names, values)] appended
    as further float properties."""
    n = len(pos)
    names = ["x", "y", "z", "red", "green", "blue", "alpha"] + [c for cols, _ in extra for c in cols]
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment created by cfd_taichi_amd\nelement vertex %d\n" % n)
        for name in names:
            f.write("property float %s\n" % name)
        f.write("end_header\n")
        np.savetxt(f, np.hstack([pos, rgba] + [np.asarray(v, dtype=np.float32).reshape(n, -1) for _, v in extra]), fmt="%.6f")


def parse_remove_geometry(items, known=None):
    """--remove-geometry NAME@FRAME (repeatable) as {frame: [names]} in the order given; known: the names the config defines.  A malformed item,
    a frame below 0, an unknown or repeated name ends the run"""
    out, seen = {}, set()
    for item in items or []:
        name, sep, frame = item.rpartition("@")
        if not sep or not name or not frame.isdigit():
            raise SystemExit("--remove-geometry: expected NAME@FRAME with FRAME >= 0, got '%s'" % item)
        if known is not None and name not in known:
            raise SystemExit("--remove-geometry: the config defines no geometry '%s' (scene.geometry has %s)" % (name, ", ".join(sorted(known)) or "none"))
        if name in seen:
            raise SystemExit("--remove-geometry: '%s' is removed twice" % name)
        seen.add(name)
        out.setdefault(int(frame), []).append(name)
    return out


def geometry_names(config):
    """the names of `scene.geometry` as the block gives them (nothing is sampled: the handle does that once, when it is made)"""
    block = config["scene"].get("geometry")
    return [e.get("name") for e in block if isinstance(e, dict)] if isinstance(block, list) else []


def unreached_removals(removals, frames):
    """the NAME@FRAME items whose frame the run never reached (`frames`: frames run; a removal at frame f happens before frame f + 1 starts)"""
    return ["%s@%d" % (name, f) for f in sorted(removals) if f >= frames for name in removals[f]]


def write_geometry_ply(path, sim, wall_species=1, f_wall_pos=32):
    """The wall samples as they stand, box and geometry, as ASCII PLY: float x y z and an int `group` column (0: the box).  wall_species /
    f_wall_pos: SPH_SPECIES_WALL / SPH_F_WALL_POS.  While loads are measured (sim.measured_groups): float fx fy fz behind them, the last step's
    force on every sample of a measured group, zero on the others"""
    pos = np.asarray(sim.download(f_wall_pos, wall_species), dtype=np.float32)
    group = np.zeros(len(pos), dtype=np.int64)
    rows = {0: (0, len(pos))}
    for g, first, count in sim.geometry():
        group[first:first + count] = g
        rows[g] = (first, count)
        rows[0] = (0, rows[0][1] - count)
    measured = list(getattr(sim, "measured_groups", []))
    force = np.zeros((len(pos), 3), dtype=np.float32)
    for g in measured:
        force[rows[g][0]:rows[g][0] + rows[g][1]] = sim.wall_forces(g)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment created by cfd_taichi_amd\nelement vertex %d\n" % len(pos))
        f.write("property float x\nproperty float y\nproperty float z\nproperty int group\n")
        if measured:
            f.write("property float fx\nproperty float fy\nproperty float fz\n")
        f.write("end_header\n")
        for k, (p, g) in enumerate(zip(pos, group)):
            f.write("%.6f %.6f %.6f %d" % (p[0], p[1], p[2], g))
            if measured:
                f.write(" %.9g %.9g %.9g" % tuple(force[k]))
            f.write("\n")


LOAD_COLUMNS = ("frame", "time", "group", "seconds", "mean_fx", "mean_fy", "mean_fz", "mean_tx", "mean_ty", "mean_tz", "fx", "fy", "fz")


def load_rows(sim, frame, t):
    """One row of LOAD_COLUMNS per measured group of `sim` (anything with measured_groups, geometry_groups, wall_impulse, wall_load) for the frame
    that just ended: the window since the last call is read and reset.  A window of no seconds gives NaN means."""
    names = {0: "box"}
    names.update({g: n for n, g in sim.geometry_groups.items()})
    rows = []
    for g in sim.measured_groups:
        j, l, sec = sim.wall_impulse(g, reset=True)
        f, _ = sim.wall_load(g)
        mean = [float(v) / sec if sec > 0 else float("nan") for v in list(j) + list(l)]
        rows.append((int(frame), float(t), names.get(g, str(g)), float(sec)) + tuple(mean) + tuple(float(v) for v in f))
    return rows


def write_load_csv(path, rows):
    """the rows of load_rows under a header of LOAD_COLUMNS.  %.17g: every f64 comes back bit for bit"""
    with open(path, "w") as f:
        f.write(",".join(LOAD_COLUMNS) + "\n")
        for r in rows:
            f.write(",".join(v if isinstance(v, str) else ("%d" % v if isinstance(v, int) else "%.17g" % v) for v in r) + "\n")


def write_diag_csv(path, chunks):
    """One line per recorded step under a header of the slot names; `chunks`: the structured arrays of Simulation.diagnostics_log(), in order.
    %.17g: every f64 comes back bit for bit."""
    from ._native import DIAG_SLOTS
    with open(path, "w") as f:
        f.write(",".join(DIAG_SLOTS) + "\n")
        for rows in chunks:
            for row in rows:
                f.write(",".join("%.17g" % row[name] for name in DIAG_SLOTS) + "\n")


def drain_diag(sim, chunks, dropped):
    """the rows recorded since the last drain onto `chunks`; returns the running count of rows lost to the ring"""
    rows, lost = sim.diagnostics_log()
    if len(rows):
        chunks.append(rows)
    return max(dropped, lost)


def main_sharded(args, config):
    """WORLD_SIZE > 1 (launched by torchrun): one x-slab per rank, native RCCL transport when every rank has its own GPU (else
    torch.distributed callbacks); rank 0 gathers the positions for the PLY frames."""
    import torch
    import torch.distributed as dist
    from . import _native as nat
    from .slab import SlabSimulation
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    if config.get("solid"):
        raise SystemExit("rigid bodies are not sharded: run this config on one GPU")
    if config["scene"].get("emitters") or config["scene"].get("sinks") or config["fluid"].get("capacity"):
        raise SystemExit("emitters, sinks and fluid.capacity are not sharded: run this config on one GPU")
    # (`scene.loads` is skipped on slab handles with a printed line -- geometry.apply_loads: loads are measured on one GPU)
    if config["scene"].get("scalar") is not None or PLY_SCALAR in args.ply_fields:
        raise SystemExit("the carried scalar (scene.scalar, --ply-fields scalar) is not sharded: run this config on one GPU")
    own_gpu = torch.cuda.device_count() >= int(os.environ.get("LOCAL_WORLD_SIZE", world))
    device = local if own_gpu else 0
    if own_gpu:
        torch.cuda.set_device(device)
        dist.init_process_group("nccl", device_id=torch.device("cuda", device))
    else:
        dist.init_process_group("gloo")
    transport = args.transport or ("native" if own_gpu else "torch")
    sim = SlabSimulation(config, rank, world, device=device, transport=transport, rebalance_every=50, arith=nat.arith_id(args.arith))
    if args.ply_fields:              # derived fields are not sharded: the library says why
        try:
            sim.sim.derived(args.ply_fields[0])
        except nat.SphError as e:
            raise SystemExit(str(e))
    scene_config, solver_config = config["scene"], config["solver"]
    iter_cnt = solver_config.get("iter_cnt")
    ply_dir = args.ply_dir or ("./output" if scene_config.get("is_output_ply", False) else None)
    if ply_dir and rank == 0:
        os.makedirs(ply_dir, exist_ok=True)
    rgba = np.tile(np.float32([0.0, 0.26, 0.68, 1.0]), (sim.n_fluid, 1))          # ParticleSystem.py:152
    frame_time = 1.0 / scene_config.get("output_fps", 60)
    frame_cnt, ply_cnt, t = 0, 0, 0.0
    start_time = time.time()
    while True:
        for name in getattr(args, "removals", {}).get(frame_cnt, []):           # every rank alike, between the same steps
            sim.remove_geometry(sim.geometry_groups[name])
        sim.step(iter_cnt)
        frame_cnt += 1
        t += iter_cnt * sim.sim.scalar(nat.S_DELTA_TIME)
        if ply_dir and (t / frame_time) > ply_cnt:
            pos = sim.gather(nat.F_POS)
            if rank == 0:
                write_ply_ascii(os.path.join(ply_dir, "output_%06d.ply" % ply_cnt), pos, rgba)
            ply_cnt += 1
        if (args.steps and frame_cnt >= args.steps) or t > args.until or frame_cnt > 100000:
            break
    if rank == 0:
        for item in unreached_removals(getattr(args, "removals", {}), frame_cnt):
            print("--remove-geometry %s: the run ended after %d frames, the geometry stayed" % (item, frame_cnt))
        print("slabs: %d, frames: %d, simulated time: %.6f s, PLY frames: %d" % (world, frame_cnt, t, ply_cnt))
        print("Simulation time: {}".format(time.time() - start_time))
    sim.close()
    dist.barrier()
    dist.destroy_process_group()
    return frame_cnt, t, ply_cnt


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="./default.json")          # main.py:14
    ap.add_argument("--solver", default=None, help="override solver.name (wcsph | dfsph | pcisph | iisph | pbf)")
    ap.add_argument("--until", type=float, default=4.0, help="stop when simulated time exceeds this (main.py:205)")
    ap.add_argument("--steps", type=int, default=0, help="stop after this many frames (0 = use --until)")
    ap.add_argument("--ply-dir", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--transport", default=None, choices=["native", "torch"], help="sharded runs: the library's own RCCL communicator (default with one GPU per rank) or torch.distributed callbacks")
    ap.add_argument("--arith", default=None, choices=["exact", "relaxed"],
                    help="exact (default): the reference's f32 operations in its order; relaxed: the tolerance-grade sweeps (SphConfig.arith)")
    ap.add_argument("--release-rigid-at", type=int, default=None, metavar="FRAME",
                    help="activate the rigid body when frame_cnt reaches FRAME (main.py:100-106: let the fluid settle first)")
    ap.add_argument("--diag-csv", default=None, metavar="PATH", help="record the fluid's run diagnostics on the device and write them as CSV at the end of the run")
    ap.add_argument("--diag-every", type=int, default=1, metavar="N", help="with --diag-csv: one row every N solver steps (default 1)")
    ap.add_argument("--ply-fields", default=None, metavar="NAMES", help="derived fields as extra PLY columns: a comma-separated choice of vorticity, divergence, normal, cover, scalar")
    ap.add_argument("--remove-geometry", action="append", default=None, metavar="NAME@FRAME",
                    help="take the scene.geometry entry NAME out of the wall set when frame_cnt reaches FRAME (repeatable): pulls a gate")
    ap.add_argument("--geometry-ply", default=None, metavar="DIR", help="write the wall samples with a group column at frame 0 and after every edit")
    ap.add_argument("--load-csv", default=None, metavar="PATH", help="write the load on every measured wall group (scene.loads), frame by frame, as CSV at the end of the run")
    args = ap.parse_args(argv)
    args.ply_fields = parse_ply_fields(args.ply_fields)
    if args.diag_csv and args.diag_every < 1:
        raise SystemExit("--diag-every must be >= 1")

    config = utils.read_config(args.config)
    if args.solver:
        config["solver"]["name"] = args.solver
    removals = parse_remove_geometry(args.remove_geometry, known=geometry_names(config))
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        if args.diag_csv:
            raise SystemExit("--diag-csv is not sharded: run this config on one GPU")
        if args.geometry_ply:
            raise SystemExit("--geometry-ply is not sharded: run this config on one GPU")
        if args.load_csv:
            raise SystemExit("--load-csv is not sharded: run this config on one GPU")
        args.removals = removals
        return main_sharded(args, config)
    scene_config, solver_config = config["scene"], config["solver"]
    print("Simulation Start!")
    start_time = time.time()
    ps = ParticleSystem(config, device=args.device, arith=args.arith)
    name = solver_config.get("name")
    if name not in ("wcsph", "dfsph", "pcisph", "iisph", "pbf"):
        raise SystemExit("solver '%s' is not covered; pass --solver wcsph | dfsph | pcisph | iisph | pbf" % name)
    module = importlib.import_module("cfd_taichi_amd." + name + "_solver")      # main.py:65-68
    solver = getattr(module, name + "_solver")(ps, config)
    rs = rigid_solver(ps, config) if config.get("solid", {}) else None           # :69-71
    iter_cnt = solver_config.get("iter_cnt")
    emitters, sinks = emitter.from_config(config)
    ply_dir = args.ply_dir or ("./output" if scene_config.get("is_output_ply", False) else None)
    if ply_dir:
        os.makedirs(ply_dir, exist_ok=True)
    np_rgba = ps.rgba.to_numpy()
    frame_time = 1.0 / scene_config.get("output_fps", 60)
    frame_cnt, ply_cnt, t = 0, 0, 0.0
    adaptive = name != "dfsph" and solver.adaptive_dt       # this package's adaptive time step: the steps of a frame differ, t is the handle's clock
    frame_dt = []
    diag_chunks, diag_dropped = [], 0
    if args.diag_csv:
        ps._sim.record_diagnostics(args.diag_every)
    load_table = []
    if args.load_csv and not ps._sim.measured_groups:
        raise SystemExit("--load-csv: the config measures no loads (scene.loads names the wall groups)")
    geo_cnt = 0
    if args.geometry_ply:
        os.makedirs(args.geometry_ply, exist_ok=True)
        write_geometry_ply(os.path.join(args.geometry_ply, "geometry_%06d.ply" % frame_cnt), ps._sim)
        geo_cnt += 1
    while True:
        if frame_cnt > 100000:                                                   # :98
            break
        for gname in removals.get(frame_cnt, []):
            ps._sim.remove_geometry(ps._sim.geometry_groups[gname])
            print("frame %d: geometry '%s' removed" % (frame_cnt, gname))
            if args.geometry_ply:
                write_geometry_ply(os.path.join(args.geometry_ply, "geometry_%06d.ply" % frame_cnt), ps._sim)
                geo_cnt += 1
        if rs and args.release_rigid_at is not None and frame_cnt == args.release_rigid_at:   # :100-106
            ps.active_rigid[None] = 1
            ps.reset_grid()
            ps.update_grid()
            ps.init_rigid_particles_data()
        for _ in range(iter_cnt):
            solver.step()
            if emitters or sinks:
                emitter.apply(ps._sim, emitters, sinks)
        for _ in range(iter_cnt):
            if rs and ps.active_rigid[None] == 1:
                rs.step()
        frame_cnt += 1
        if args.diag_csv:
            diag_dropped = drain_diag(ps._sim, diag_chunks, diag_dropped)
        frame_dt.append(solver.delta_time[None])
        t = solver.time[None] if adaptive else t + iter_cnt * frame_dt[-1]
        if args.load_csv:
            load_table += load_rows(ps._sim, frame_cnt, t)
        if ply_dir and (t / frame_time) > ply_cnt:                               # :189
            if len(np_rgba) != ps.particle_num:                                   # an emitter or a sink changed the count
                np_rgba = ps.rgba.to_numpy()
            write_ply_ascii(os.path.join(ply_dir, "output_%06d.ply" % ply_cnt), ps.fluid_particles.pos.to_numpy(), np_rgba, ply_extra(ps._sim, args.ply_fields))
            if ps.exist_rigid[None] == 1:                                        # :196-200
                ps.update_mesh_vextics()
                with open(os.path.join(ply_dir, "obj_%06d.obj" % ply_cnt), "w") as f:
                    f.write(ps.mesh.export(file_type="obj"))
            ply_cnt += 1
        if (args.steps and frame_cnt >= args.steps) or t > args.until:           # :205
            break
    if args.diag_csv:
        ps._sim.record_diagnostics(0)
        write_diag_csv(args.diag_csv, diag_chunks)
        print("diagnostics: %d rows in %s%s" % (sum(len(c) for c in diag_chunks), args.diag_csv, ", %d lost to the ring" % diag_dropped if diag_dropped else ""))
    if args.load_csv:
        write_load_csv(args.load_csv, load_table)
        print("loads: %d rows in %s" % (len(load_table), args.load_csv))
    for item in unreached_removals(removals, frame_cnt):
        print("--remove-geometry %s: the run ended after %d frames, the geometry stayed" % (item, frame_cnt))
    print("frames: %d, simulated time: %.6f s, PLY frames: %d" % (frame_cnt, t, ply_cnt))
    print("Simulation time: {}".format(time.time() - start_time))               # :211
    LAST.update(ps=ps, solver=solver, rigid=rs, emitters=emitters, sinks=sinks, frame_dt=frame_dt, geometry_frames=geo_cnt)      # frame_dt: delta_time after every frame
    return frame_cnt, t, ply_cnt


if __name__ == "__main__":
    main()
