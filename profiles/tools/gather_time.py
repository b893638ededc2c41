"""Time of an entity gather compute (mwhip_gather_compute_async) at the BASELINE
configs[2] shape -- escape_room_phys, 8192 worlds, after 50 steps: Position,
Rotation and Velocity of every agent's partner (what Agent.OtherAgents holds)
and of every door's four buttons (Entity buttons[4] inside the 40-byte
DoorProperties cells, read through a world view's slab; unused slots hold
Entity::none()) -- next to two lower bounds that resolve no handle:
  (a) the two gather computes, queued back to back; (a1), (a2) each alone;
  (b) torch.index_select of the same cells (those of the handles that name an
      entity, from world-view slabs of the tables) by rows precomputed on the
      host;
  (c) ONE contiguous device-to-device hipMemcpyAsync of the bytes (a) writes
      into its component buffers.
escape_room_phys does not list Agent.OtherAgents among the columns a world view
can name, so the same handles -- for each agent the other agent of its world --
are built from Agent.Entity and gathered through a device tensor.
Every figure is the median of REPS repetitions, each timed with a pair of HIP
events on the executor's own stream around the calls named, after WARM untimed
repetitions of the same call.  The state is the same for all of them; between
repetitions the stream is idle.  Writes profiles/gather_times.md:
    python profiles/tools/gather_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.gather_ref import read_handles
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "gather_times.md")
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
        raise SystemExit("gather_time.py measures on the GPU; none is visible")
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
        names = [c[0] for c in sim.columns]
        per_world = {t: sim.dump_column(names.index(t + ".Entity"), 512)[1]
                     for t in ("Agent", "ButtonEntity", "DoorEntity")}
        assert (per_world["Agent"] == 2).all()
        doors_max, buttons_max = (int(per_world[t].max()) for t in ("DoorEntity", "ButtonEntity"))

        with sim.world_view("Agent", ["Agent.Entity"] + ["Agent." + c for c in COMPONENTS],
                            max_rows=2) as agents, \
                sim.world_view("ButtonEntity", ["ButtonEntity.Entity", "ButtonEntity.Position"],
                               max_rows=buttons_max) as buttons, \
                sim.world_view("DoorEntity", ["DoorEntity.DoorProperties"],
                               max_rows=doors_max) as doors:
            for view in (agents, buttons, doors):
                view.compute()
            # each agent's partner: the other Entity cell of its world
            partners = agents.tensor("Agent.Entity").reshape(W, 2, 8).flip(1).contiguous()
            door_source = doors.handle_source("DoorEntity.DoorProperties", 0, 4)
            with sim.entity_gather(partners, COMPONENTS) as through_agents, \
                    sim.entity_gather(door_source, COMPONENTS) as through_doors:
                gathers = (through_agents, through_doors)

                def both():
                    through_agents.compute_async()
                    through_doors.compute_async()

                results = [("(a) both gather computes", timed(stream, both)),
                           ("(a1) the partners' gather alone",
                            timed(stream, through_agents.compute_async)),
                           ("(a2) the doors' buttons' gather alone",
                            timed(stream, through_doors.compute_async))]
                sim.sync()
                named = [int((g.archetypes >= 0).sum().item()) for g in gathers]
                cell_bytes = sum(through_agents.cell_bytes(c) for c in COMPONENTS)
                written = sum(g.num_handles for g in gathers) * cell_bytes
                assert named[0] == 2 * W

                # (b): rows precomputed on the host, then index_select per column
                def rows_of(view, column, handles):
                    ents = read_handles(view.tensor(column).cpu().numpy(),
                                        W * view.max_rows, 8)
                    where = {(int(g), int(i)): r for r, (g, i) in enumerate(ents.tolist())
                             if i < 2 ** 31}
                    rows = [where.get((int(g), int(i)), -1) for g, i in handles.tolist()]
                    return np.array(rows, dtype=np.int64)

                agent_rows = rows_of(agents, "Agent.Entity",
                                     read_handles(partners.cpu().numpy(), 2 * W, 8))
                door_handles = read_handles(
                    doors.tensor("DoorEntity.DoorProperties").cpu().numpy(), *door_source[1:])
                button_rows = rows_of(buttons, "ButtonEntity.Entity", door_handles)
                assert (agent_rows >= 0).all() and int((button_rows >= 0).sum()) == named[1]
                agent_index = torch.from_numpy(agent_rows).to(device)
                button_index = torch.from_numpy(button_rows[button_rows >= 0]).to(device)
                tables = [(agents.tensor("Agent." + c).reshape(2 * W, -1), agent_index)
                          for c in COMPONENTS]
                tables.append((buttons.tensor("ButtonEntity.Position")
                               .reshape(W * buttons_max, -1), button_index))
                outs = [torch.empty((len(i), t.shape[1]), dtype=torch.uint8, device=device)
                        for t, i in tables]
                selected = sum(o.numel() for o in outs)
                ext = torch.cuda.ExternalStream(stream.value, device=device)

                def select():
                    with torch.cuda.stream(ext):
                        for (table, index), out in zip(tables, outs):
                            torch.index_select(table, 0, index, out=out)

                results.append(("(b) torch.index_select of the same cells, rows precomputed "
                                "on the host", timed(stream, select)))
                sim.sync()
                got = through_agents.tensor("Position").cpu().numpy()
                assert np.array_equal(got, outs[0].cpu().numpy()), "(a) and (b) disagree"
                got = through_doors.tensor("Position").cpu().numpy()[button_rows >= 0]
                assert np.array_equal(got, outs[3].cpu().numpy()), "(a) and (b) disagree"

                src = torch.empty(written, dtype=torch.uint8, device=device)
                dst = torch.empty(written, dtype=torch.uint8, device=device)
                results.append((
                    "(c) one contiguous hipMemcpyAsync of the bytes (a) writes",
                    timed(stream, lambda: hip_check(
                        hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), written, D2D, stream),
                        "hipMemcpyAsync"))))
                handles = [g.num_handles for g in gathers]

    device_name = (f"{torch.cuda.get_device_name(0)} "
                   f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    lines = [
        "# Entity gathers: compute times",
        "",
        f"Written by `profiles/tools/gather_time.py` on: {device_name}.",
        "",
        f"Shape: `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after {STEPS} steps "
        f"(BASELINE configs[2]); Position, Rotation and Velocity ({cell_bytes} bytes per handle) "
        f"through {handles[0]} handles of agents' partners (a device tensor built from "
        f"Agent.Entity: the simulator does not list Agent.OtherAgents; all of them name an "
        f"agent) and through {handles[1]} handles of doors' buttons (4 per 40-byte "
        f"DoorProperties cell of a world view's slab, {doors_max} cells per world; {named[1]} "
        f"name a button, whose table has Position only, the others are Entity::none() or "
        f"padding).",
        f"(a) writes {written} bytes of cells and {8 * sum(handles)} bytes of archetype and "
        f"world; (b) selects {selected} bytes.",
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
    lines += ["", "Reported, not gated.  (b) and (c) resolve no handle: (b) is four launches "
              "that read rows the host looked up, (c) moves the bytes and nothing else.", ""]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
