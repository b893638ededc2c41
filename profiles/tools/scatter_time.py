"""Time of an entity scatter apply (mwhip_scatter_apply_async, three launches) at
the BASELINE configs[2] shape -- escape_room_phys, 8192 worlds, after 50 steps:
Position, Rotation and Velocity written into every agent's partner and into
every door's four buttons, through the handles of profiles/tools/gather_time.py
(the partners' built from Agent.Entity and scattered through a device tensor;
the buttons' read from the 40-byte DoorProperties cells of a world view's slab,
unused slots Entity::none()) -- next to
  (a) the apply of each scatter, everything selected; what it stores is what a
      gather through the same handles has just read, so the state stays what it is;
  (b) ONE contiguous device-to-device hipMemcpyAsync of the bytes (a) writes
      into the tables, as the floor;
  (c) the torch route a user has without scatters: a world view of the table
      (Entity and the columns), a search per handle (torch.sort of the view's
      Entity cells as int64 keys, torch.searchsorted of the handles), the
      view's slabs copied into a world write's, an indexed assignment per
      column (rows the search missed get their own value back), and the world
      write's apply;
and one step scatter's three launches in mwhip_profile next to the step's
other launches.  Every figure of (a) to (c) is the median of REPS repetitions,
each timed with a pair of HIP events on the executor's own stream around the
calls named, after WARM untimed repetitions of the same call; between
repetitions the stream is idle.  Writes profiles/scatter_times.md:
    python profiles/tools/scatter_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "scatter_times.md")
SIM, STEPS, DENOM, SEED = "escape_room_phys", 50, 200, 5
COMPONENTS = ["Position", "Rotation", "Velocity"]
REPS, WARM = 20, 3
D2D = 3     # hipMemcpyDeviceToDevice


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("scatter_time.py measures on the GPU; none is visible")
    runtime_lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_check(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_check(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def timed(stream, fn):
        times = []
        for rep in range(WARM + REPS):
            hip_check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            hip_check(hip.hipEventRecord(ev0, stream), "hipEventRecord")
            fn()
            hip_check(hip.hipEventRecord(ev1, stream), "hipEventRecord")
            hip_check(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
            ms = C.c_float(0)
            hip_check(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
            if rep >= WARM:
                times.append(ms.value * 1e3)
        return statistics.median(times), min(times), max(times)

    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=DENOM) as sim:
        sim.step(STEPS)
        stream = C.c_void_p(sim.stream())
        device = torch.device("cuda", sim.gpu_id)
        ext = torch.cuda.ExternalStream(stream.value, device=device)
        names = [c[0] for c in sim.columns]
        per_world = {t: sim.dump_column(names.index(t + ".Entity"), 512)[1]
                     for t in ("Agent", "ButtonEntity", "DoorEntity")}
        assert (per_world["Agent"] == 2).all()
        doors_max, buttons_max = (int(per_world[t].max()) for t in ("DoorEntity", "ButtonEntity"))
        agent_columns = ["Agent." + c for c in COMPONENTS]
        digest = sim.digest()
        state = digest.compute().copy()

        with sim.world_view("Agent", ["Agent.Entity"] + agent_columns, max_rows=2) as agents, \
                sim.world_view("ButtonEntity", ["ButtonEntity.Entity", "ButtonEntity.Position"],
                               max_rows=buttons_max) as buttons, \
                sim.world_view("DoorEntity", ["DoorEntity.DoorProperties"],
                               max_rows=doors_max) as doors, \
                sim.world_write("Agent", agent_columns, max_rows=2) as agent_write, \
                sim.world_write("ButtonEntity", ["ButtonEntity.Position"],
                                max_rows=buttons_max) as button_write:
            for view in (agents, buttons, doors):
                view.compute()
            # each agent's partner: the other Entity cell of its world
            partners = agents.tensor("Agent.Entity").reshape(W, 2, 8).flip(1).contiguous()
            door_source = doors.handle_source("DoorEntity.DoorProperties", 0, 4)
            with sim.entity_gather(partners, COMPONENTS) as agents_in, \
                    sim.entity_gather(door_source, COMPONENTS) as doors_in, \
                    sim.entity_scatter(partners, COMPONENTS) as through_agents, \
                    sim.entity_scatter(door_source, COMPONENTS) as through_doors:
                scatters = (through_agents, through_doors)
                for gather, scatter in ((agents_in, through_agents), (doors_in, through_doors)):
                    gather.compute()
                    for c in COMPONENTS:
                        scatter.tensor(c).copy_(gather.tensor(c))
                    scatter.select.fill_(1)
                torch.cuda.synchronize()

                results = [("(a1) the partners' scatter apply, three launches",
                            timed(stream, through_agents.apply_async)),
                           ("(a2) the doors' buttons' scatter apply, three launches",
                            timed(stream, through_doors.apply_async))]
                sim.sync()
                handles = [s.num_handles for s in scatters]
                named = [int((s.archetypes >= 0).sum().item()) for s in scatters]
                won = [int(s.written.sum().item()) for s in scatters]
                cell_bytes = sum(through_agents.cell_bytes(c) for c in COMPONENTS)
                position_bytes = through_agents.cell_bytes("Position")
                assert named[0] == won[0] == 2 * W
                assert np.array_equal(digest.compute(), state), "(a) changed the state"
                # (the buttons' table has Position only)
                stored = [won[0] * cell_bytes, won[1] * position_bytes]

                for label, nbytes in (("(b1) one contiguous hipMemcpyAsync of the bytes (a1) "
                                       "stores", stored[0]),
                                      ("(b2) one contiguous hipMemcpyAsync of the bytes (a2) "
                                       "stores", stored[1])):
                    src = torch.empty(nbytes, dtype=torch.uint8, device=device)
                    dst = torch.empty(nbytes, dtype=torch.uint8, device=device)
                    results.append((label, timed(stream, lambda: hip_check(
                        hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, D2D, stream),
                        "hipMemcpyAsync"))))

                # (c): view, search per handle, indexed assignment per column, write
                def keys_of(cells):
                    return cells.reshape(-1, 8).view(torch.int64).reshape(-1)

                def torch_route(view, write, entity, columns, handle_keys, values):
                    def run():
                        view.compute_async()
                        with torch.cuda.stream(ext):
                            keys, order = torch.sort(keys_of(view.tensor(entity)))
                            at = torch.searchsorted(keys, handle_keys).clamp_(max=len(keys) - 1)
                            hit = (keys[at] == handle_keys).unsqueeze(1)
                            rows = order[at]
                            for column, cells in zip(columns, values):
                                slab = write.tensor(column).reshape(len(keys), -1)
                                slab.copy_(view.tensor(column).reshape(len(keys), -1))
                                slab.index_copy_(0, rows, torch.where(hit, cells, slab[rows]))
                        write.apply_async()
                    return run

                agent_write.take.fill_(2)
                button_write.take.fill_(buttons_max)
                door_keys = keys_of(torch.from_numpy(np.ascontiguousarray(
                    doors.tensor("DoorEntity.DoorProperties").cpu().numpy()
                    .reshape(-1, 40)[:, :32])).to(device))
                torch.cuda.synchronize()
                results.append((
                    "(c1) the partners through torch: view, sort + searchsorted, index_copy_ "
                    "per column, world write",
                    timed(stream, torch_route(agents, agent_write, "Agent.Entity", agent_columns,
                                              keys_of(partners),
                                              [through_agents.tensor(c) for c in COMPONENTS]))))
                results.append((
                    "(c2) the doors' buttons through torch, likewise (Position only)",
                    timed(stream, torch_route(buttons, button_write, "ButtonEntity.Entity",
                                              ["ButtonEntity.Position"], door_keys,
                                              [through_doors.tensor("Position")]))))
                sim.sync()
                assert np.array_equal(digest.compute(), state), "(c) changed the state"

                # one step scatter inside the step
                through_agents.every_step()
                launches = sim.profile(REPS)
                through_agents.every_step(False)
        digest.close()

    step_us = sum(k["avg_us"] for k in launches)
    scatter_launches = [k for k in launches if k["name"].startswith("scatter:")]
    assert len(scatter_launches) == 3
    device_name = (f"{torch.cuda.get_device_name(0)} "
                   f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    by_name = dict(results)
    lines = [
        "# Entity scatters: apply times",
        "",
        f"Written by `profiles/tools/scatter_time.py` on: {device_name}.",
        "",
        f"Shape: `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after {STEPS} steps "
        f"(BASELINE configs[2]); Position, Rotation and Velocity ({cell_bytes} bytes per handle) "
        f"through {handles[0]} handles of agents' partners (a device tensor built from "
        f"Agent.Entity; all of them name an agent and all win: {stored[0]} bytes stored) and "
        f"through {handles[1]} handles of doors' buttons (4 per 40-byte DoorProperties cell of a "
        f"world view's slab, {doors_max} cells per world; {named[1]} name a button, {won[1]} "
        f"win, the button table has Position only: {stored[1]} bytes stored; the others are "
        f"Entity::none() or padding).  Everything is selected; the cells are those a gather "
        f"through the same handles has just read, so no apply changes the state (the digest "
        f"is checked).  Claim tables: {8 * 2 * handles[0]} and {8 * 2 * handles[1]} bytes.",
        "",
        f"Median of {REPS} (min - max), after {WARM} untimed repetitions; each repetition "
        "is timed with two HIP events on the executor's stream around the calls named, "
        "with the stream idle before it.",
        "",
        "| what | median us | min - max us |",
        "|---|---:|---:|",
    ]
    for name, (med, lo, hi) in results:
        lines.append(f"| {name} | {med:.1f} | {lo:.1f} - {hi:.1f} |")
    ratios = []
    for k in ("1", "2"):
        a = next(v[0] for n, v in by_name.items() if n.startswith(f"(a{k})"))
        b = next(v[0] for n, v in by_name.items() if n.startswith(f"(b{k})"))
        c = next(v[0] for n, v in by_name.items() if n.startswith(f"(c{k})"))
        ratios.append(f"(a{k}) is {a / b:.2f} x (b{k}) and {a / c:.3f} x (c{k})")
    lines += ["", "Ratios of the medians: " + "; ".join(ratios) + ".",
              "Reported, not gated.  (b) resolves no handle and moves the bytes and nothing "
              "else.  (c) is what a user without scatters queues on the same stream; it "
              "resolves duplicates in no defined order.",
              "",
              f"One step scatter (the partners') inside the step, `mwhip_profile`, mean of "
              f"{REPS} replays, kernel time between HIP events per launch: the step's "
              f"{len(launches)} launches take {step_us:.1f} us, of which",
              "",
              "| launch | mean us | algo bytes |",
              "|---|---:|---:|"]
    for k in scatter_launches:
        lines.append(f"| {k['name']} | {k['avg_us']:.1f} | {int(k['algo_bytes'])} |")
    lines += ["", "The five longest other launches of that step: " + ", ".join(
        f"{k['name']} {k['avg_us']:.1f}" for k in sorted(
            (k for k in launches if not k["name"].startswith("scatter:")),
            key=lambda k: -k["avg_us"])[:5]) + " us.", ""]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
