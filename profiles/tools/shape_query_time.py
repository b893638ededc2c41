"""Time of a shape query compute (mwhip_shapes_compute_async) on
escape_room_phys, 8192 worlds, after 50 steps: one bundle per world with two
shapes, each agent's own collision object at the agent's pose displaced along
its last action (a quarter of a unit per unit of move amount, at the action's
angle in the agent's frame), exclude = the agent, read from a world view's slab
of the Entity column; 8 hit slots per shape.  Both mappings (cooperative, the
default, and plain -- every pair through the generic single-lane routine, one at
a time); their words are compared before anything is timed.  Next to them the
current-pose contact query of the same run (32 slots per world) and the physics
step kernels of the same simulator from mwhip_profile (the average of 20
profiled steps): context, not bars.
Each figure is the median of REPS repetitions, each timed with a pair of HIP
events on the executor's own stream around one compute_async, after WARM untimed
repetitions, with the stream idle in between.  No threshold.  Writes
profiles/shape_query_times.md:
    python profiles/tools/shape_query_time.py [worlds] [out.md]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from madrona_amd.simlib import Simulator, hip_lib_path, runtime_lib

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles",
                                                         "shape_query_times.md")
SIM, STEPS, DENOM, SEED = "escape_room_phys", 50, 200, 5
AGENTS, K, CONTACT_K = 2, 8, 32
AGENT_OBJECT, NUM_OBJECTS = 3, 6        # sims/escape_room_phys/sim.hpp: SimObject
REPS, WARM = 20, 3


def hip_check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> hipError {rc}")


def rotate(q, v):
    """v rotated by the unit quaternions q (w, x, y, z), row by row"""
    w, u = q[:, :1], q[:, 1:]
    t = 2 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def main():
    import torch    # (its HIP runtime is the one every library of the process binds to)
    if not torch.cuda.is_available():
        raise SystemExit("shape_query_time.py measures on the GPU; none is visible")
    runtime_lib()
    hip = C.CDLL("libamdhip64.so")
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

    rows = []
    rng = np.random.default_rng(SEED)
    with Simulator(hip_lib_path(SIM), W, seed=SEED, flags=DENOM) as sim, \
            sim.world_view("Agent", ["Agent.Entity", "Agent.Position", "Agent.Rotation",
                                     "Agent.Action"], max_rows=AGENTS) as view:
        for _ in range(STEPS):
            action = np.stack([rng.integers(0, 4, (W, AGENTS)), rng.integers(0, 8, (W, AGENTS)),
                               rng.integers(-2, 3, (W, AGENTS)), np.zeros((W, AGENTS), int)],
                              -1).astype(np.int32)
            sim.write_tensor("action", action)
            sim.step(1)
        stream = C.c_void_p(sim.stream())
        view.compute()
        torch.cuda.synchronize()
        assert (view.counts.cpu().numpy() == AGENTS).all()
        position = view.tensor("Agent.Position", np.float32).cpu().numpy().reshape(-1, 3)
        rotation = view.tensor("Agent.Rotation", np.float32).cpu().numpy().reshape(-1, 4)
        last = view.tensor("Agent.Action", np.int32).cpu().numpy().reshape(W * AGENTS, -1)
        angle = 2 * np.pi * last[:, 1] / 8
        local = 0.25 * last[:, :1] * np.stack([np.sin(angle), np.cos(angle), 0 * angle], 1)
        posed = (position + rotate(rotation, local.astype(np.float32))).astype(np.float32)

        outs = {}
        for plain in (False, True):
            with sim.shape_query(W, AGENTS, K, NUM_OBJECTS, bundles_per_world=1,
                                 exclude=(view.buffer_ptr("Agent.Entity"), 8, 0),
                                 plain=plain) as query:
                query.objects().fill_(AGENT_OBJECT)
                query.positions().copy_(torch.from_numpy(posed).cuda())
                query.rotations().copy_(torch.from_numpy(rotation).cuda())
                torch.cuda.synchronize()
                query.compute()
                torch.cuda.synchronize()
                outs[plain] = [t.cpu().numpy() for t in (
                    query.status(), query.counts(), query.hits(), query.shape_is_ref(),
                    query.num_points(), query.normals(), query.points())]
                assert (outs[plain][0] == 0).all()
                rows.append(("shape query, " + ("plain" if plain else "cooperative"),
                             int(outs[plain][1].sum()), int(outs[plain][1].max()),
                             timed(stream, query.compute_async)))
                sim.sync()
        for a, b in zip(outs[False], outs[True]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
                "the two mappings disagree"
        with sim.contact_query(CONTACT_K, poses="current") as contacts:
            contacts.compute()
            torch.cuda.synchronize()
            counts = contacts.counts().cpu().numpy()
            rows.append(("contact query, current poses, cooperative", int(counts.sum()),
                         int(counts.max()), timed(stream, contacts.compute_async)))
            sim.sync()
        stats = sim.profile(20)
        step = [k for k in stats if "physics:worldStep" in k["name"]]
        assert step, [k["name"] for k in stats]

    device_name = (f"{torch.cuda.get_device_name(0)} "
                   f"({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})")
    lines = [
        "# Shape queries: compute time",
        "",
        f"Written by `profiles/tools/shape_query_time.py` on: {device_name}.",
        "",
        f"Shape: `{SIM}`, {W} worlds, seed {SEED}, auto-reset 1/{DENOM}, after {STEPS} steps of "
        f"random actions; one bundle per world with {AGENTS} shapes, each agent's collision "
        "object at the agent's pose displaced along its last action, the agent excluded "
        f"through a world view's Entity slab; {K} hit slots per shape.  The two mappings' "
        "status, count, hits, shape_is_ref, num_points, normal and points are equal word for "
        "word.",
        "",
        f"Each query: median of {REPS} (min - max), after {WARM} untimed repetitions, each timed "
        "with two HIP events on the executor's stream around one compute_async, the stream "
        "idle before it.  The step kernels: their avg_us in mwhip_profile over 20 profiled "
        "steps of the same simulator (the parent commit's: this change does not touch them).",
        "",
        "| what | hits / contacts | most of a shape / in a world | us | min - max us |",
        "|---|---:|---:|---:|---:|"]
    for what, total, most, (med, lo, hi) in rows:
        lines.append(f"| {what} | {total} | {most} | {med:.1f} | {lo:.1f} - {hi:.1f} |")
    for k in step:
        lines.append(f"| `{k['name']}` in the step (mwhip_profile) | | | {k['avg_us']:.1f} | |")
    lines += [
        "",
        "Reported, not gated.  A shape query tests 2 shapes against all bodies of a world "
        f"once; the contact query ({CONTACT_K} slots per world) tests all body pairs of a "
        "world once; a step runs the narrowphase once per substep (four times) on the "
        "broadphase's candidates and solves: context, not bars.  The plain mapping sends the "
        "pairs through the generic routine one lane at a time: it is the yardstick, not a "
        "fast path.", ""]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
