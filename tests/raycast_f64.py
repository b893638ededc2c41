"""The batch ray caster's image by its definition, in float64 and without any
acceleration structure: what madrona_amd/csrc/render_raycast.hip's header says
is reproduced, restated from that description alone.  Test infrastructure only.

  primary rays   raycast_utils.primary_rays for any view rotation
  per instance   the ray goes to object space by the inverse TRS and is
                 renormalised; Moeller-Trumbore against EVERY triangle of the
                 object, back faces culled; t back in world units, in
                 (0, 10000]; the closest hit wins
  colour         override colour, or override material, or the mesh's material,
                 or the triangle's; a textured material samples its texture at
                 the interpolated (u, 1 - v) -- wrap addressing, bilinear with 8
                 fractional bits -- times the material's colour
  normal         the object-space face normal rotated by the instance's rotation
  lights         directional: -direction, unnormalised; spot: the direction to
                 the light, inside the cone by acos; a shadow-casting light
                 counts only where dir . n > 0 and no front face of any instance
                 lies along the shadow ray; contribution clamp(n . dir, 0, 1);
                 `active` and `intensity` are ignored
  pixel          min(1, max(0.2, sum) * colour) truncated to 8 bits; a miss is
                 depth 0, black, alpha 255

Every pixel is also traced with four rays displaced by +-1e-3 pixel in u and v.
It is DECIDED when all five agree on every discrete outcome (hit or miss,
instance and triangle, and per light: outside the cone / facing away /
shadowed / lit): there fp32 rounding cannot legitimately change the picture.
Depth and colour are the centre ray's."""
import numpy as np

from raycast_utils import INSTANCE_DT, LIGHT_DT, VIEW_DT

T_MAX = 10000.0
DELTA = 1e-3            # pixels
# per-light outcome of a hit
OUT_OF_CONE, FACING_AWAY, SHADOWED, LIT = 0, 1, 2, 3


def _rotate(q, v):
    """v [..., 3] rotated by the quaternion q = (w, x, y, z)"""
    w, p = q[0], q[1:]
    a = np.cross(p, v)
    return v + 2.0 * (w * a + np.cross(p, a))


def _conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def view_rays(view, res, du=0.0, dv=0.0):
    """origin [3], directions [res, res, 3] (row = pixel y) through the pixel
    centres displaced by (du, dv) pixels"""
    q = _conj(np.asarray(view["rotation"], np.float64))   # the record holds the inverse
    start = np.asarray(view["position"], np.float64)
    forward = _rotate(q, np.array([0.0, 1.0, 0.0]))
    forward /= np.linalg.norm(forward)
    u = _rotate(q, np.array([1.0, 0.0, 0.0]))
    v = np.cross(forward, u)
    v /= np.linalg.norm(v)
    viewport = 2.0 / (-float(view["yScale"]))
    horizontal, vertical = u * viewport, v * viewport
    lower_left = -horizontal / 2 - vertical / 2 + forward
    pu = (np.arange(res) + 0.5 + du) / res
    pv = (np.arange(res) + 0.5 + dv) / res
    d = (lower_left[None, None, :] + pu[None, :, None] * horizontal[None, None, :] +
         pv[:, None, None] * vertical[None, None, :])
    return start, d / np.linalg.norm(d, axis=-1, keepdims=True)


class _Object:
    def __init__(self, geo, o):
        v = geo.vertices[geo.vertex_offsets[o]:geo.vertex_offsets[o + 1]].astype(np.float64)
        self.first = int(geo.triangle_offsets[o])
        idx = geo.indices[self.first:geo.triangle_offsets[o + 1]].astype(np.int64)
        self.verts = v
        self.v0, self.e1, self.e2 = v[idx[:, 0]], v[idx[:, 1]] - v[idx[:, 0]], \
            v[idx[:, 2]] - v[idx[:, 0]]
        n = np.cross(self.e1, self.e2)
        self.normal = n / np.linalg.norm(n, axis=1, keepdims=True)
        if geo.vertex_uvs is not None:
            uv = geo.vertex_uvs[geo.vertex_offsets[o]:geo.vertex_offsets[o + 1]].astype(np.float64)
            self.uv = uv[idx]                      # [T, 3, 2]
        else:
            self.uv = np.zeros((len(idx), 3, 2))


class Scene:
    """One world's instances over the shared geometry."""

    def __init__(self, geo, instances):
        self.geo = geo
        self.inst = np.ascontiguousarray(instances).view(INSTANCE_DT).ravel()
        self.objects = {}
        self.boxes = []
        for i in self.inst:
            o = int(i["objectID"])
            if o not in self.objects:
                self.objects[o] = _Object(geo, o)
            # exact world box of the instance's vertices: a conservative prefilter
            w = _rotate(i["rotation"].astype(np.float64),
                        self.objects[o].verts * i["scale"].astype(np.float64)) + \
                i["position"].astype(np.float64)
            self.boxes.append((w.min(0) - 1e-6, w.max(0) + 1e-6))

    def trace(self, org, d):
        """Closest hit of the rays org [N,3] + t d [N,3], t in (0, T_MAX] measured
        in units of |d|.  Returns t (inf on a miss), instance, triangle (index
        into the geometry's triangle list) and the barycentric (u, v)."""
        n = len(org)
        best_t = np.full(n, np.inf)
        best_i = np.full(n, -1, np.int64)
        best_tri = np.full(n, -1, np.int64)
        best_uv = np.zeros((n, 2))
        for k, inst in enumerate(self.inst):
            lo, hi = self.boxes[k]
            with np.errstate(divide="ignore", invalid="ignore"):
                t0, t1 = (lo - org) / d, (hi - org) / d
            near = np.nanmax(np.minimum(t0, t1), -1)
            far = np.nanmin(np.maximum(t0, t1), -1)
            inside = ((org >= lo) & (org <= hi)) | (d != 0)     # d == 0: inside the slab?
            sel = np.flatnonzero((near <= far) & (far > 0) & inside.all(-1))
            if sel.size == 0:
                continue
            obj = self.objects[int(inst["objectID"])]
            q_inv = _conj(inst["rotation"].astype(np.float64))
            inv_scale = 1.0 / inst["scale"].astype(np.float64)
            for at in range(0, sel.size, 2048):
                s = sel[at:at + 2048]
                o = _rotate(q_inv, org[s] - inst["position"].astype(np.float64)) * inv_scale
                dd = _rotate(q_inv, d[s]) * inv_scale
                t_scale = np.linalg.norm(dd, axis=1)
                dd = dd / t_scale[:, None]
                pv = np.cross(dd[:, None, :], obj.e2[None])
                det = (obj.e1[None] * pv).sum(-1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    inv = 1.0 / det
                    tv = o[:, None, :] - obj.v0[None]
                    u = (tv * pv).sum(-1) * inv
                    qv = np.cross(tv, obj.e1[None])
                    v = (dd[:, None, :] * qv).sum(-1) * inv
                    t = (obj.e2[None] * qv).sum(-1) * inv / t_scale[:, None]
                    ok = (det > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & \
                        (t <= T_MAX)
                t = np.where(ok, t, np.inf)
                tri = t.argmin(1)
                rows = np.arange(len(s))
                t_min = t[rows, tri]
                closer = t_min < best_t[s]
                w = s[closer]
                best_t[w] = t_min[closer]
                best_i[w] = k
                best_tri[w] = obj.first + tri[closer]
                best_uv[w, 0] = u[rows, tri][closer]
                best_uv[w, 1] = v[rows, tri][closer]
        return best_t, best_i, best_tri, best_uv

    # ---- shading ----------------------------------------------------------------
    def _texture(self, tex, x, y):
        width, height, texels = self.geo.textures[tex]
        px = np.frombuffer(bytes(texels), np.uint8).reshape(height, width, 4)[..., :3] / 255.0
        xb, yb = x * width - 0.5, y * height - 0.5
        xf, yf = np.floor(xb), np.floor(yb)
        a = np.floor((xb - xf) * 256.0 + 0.5) / 256.0
        b = np.floor((yb - yf) * 256.0 + 0.5) / 256.0
        i0, i1 = xf.astype(np.int64) % width, (xf.astype(np.int64) + 1) % width
        j0, j1 = yf.astype(np.int64) % height, (yf.astype(np.int64) + 1) % height
        a, b = a[:, None], b[:, None]
        return ((1 - a) * (1 - b) * px[j0, i0] + a * (1 - b) * px[j0, i1] +
                (1 - a) * b * px[j1, i0] + a * b * px[j1, i1])

    def colour(self, inst_idx, tri, bary):
        geo = self.geo
        out = np.ones((len(inst_idx), 3))
        for k in np.unique(inst_idx):
            rows = np.flatnonzero(inst_idx == k)
            inst = self.inst[k]
            mat = int(inst["matID"])
            if mat == -2:
                c = int(inst["color"])
                out[rows] = [((c >> 16) & 255) / 255.0, ((c >> 8) & 255) / 255.0,
                             (c & 255) / 255.0]
                continue
            if mat == -1:
                mat = int(geo.object_materials[int(inst["objectID"])])
            mats = np.full(len(rows), mat)
            if mat == -1 and geo.triangle_materials is not None:
                mats = geo.triangle_materials[tri[rows]].astype(np.int64)
            obj = self.objects[int(inst["objectID"])]
            for m in np.unique(mats):
                if m < 0:
                    continue            # no material: white
                r = rows[mats == m]
                out[r] = geo.material_colors[m].astype(np.float64)
                tex = -1 if geo.material_textures is None else int(geo.material_textures[m])
                if tex >= 0:
                    uv = obj.uv[tri[r] - obj.first]             # [n, 3, 2]
                    bu, bv = bary[r, 0:1], bary[r, 1:2]
                    st = (1 - bu - bv) * uv[:, 0] + bu * uv[:, 1] + bv * uv[:, 2]
                    out[r] *= self._texture(tex, st[:, 0], 1.0 - st[:, 1])
        return out

    def shade(self, org, d, t, inst_idx, tri, bary, lights, drop_light=None):
        """Per hit: the light sum's discrete states [N, L] and the shaded colour."""
        n = len(t)
        lights = np.ascontiguousarray(lights).view(LIGHT_DT).ravel()
        states = np.zeros((n, len(lights)), np.int8)
        normal = np.zeros((n, 3))
        for k in np.unique(inst_idx):
            m = inst_idx == k
            inst = self.inst[k]
            obj = self.objects[int(inst["objectID"])]
            normal[m] = _rotate(inst["rotation"].astype(np.float64),
                                obj.normal[tri[m] - obj.first])
        pos = org + t[:, None] * d
        total = np.zeros(n)
        for li, light in enumerate(lights):
            direction = light["direction"].astype(np.float64)
            inside = np.ones(n, bool)
            if light["type"]:
                to_light = np.broadcast_to(-direction, (n, 3)).copy()
            else:
                to_light = light["position"].astype(np.float64) - pos
                to_light /= np.linalg.norm(to_light, axis=1, keepdims=True)
                if float(light["cutoff"]) != -1.0:
                    c = (-to_light) @ direction / np.linalg.norm(direction)
                    inside = np.abs(np.arccos(np.clip(c, -1, 1))) <= abs(float(light["cutoff"]))
            lambert = np.clip((normal * to_light).sum(-1), 0.0, 1.0)
            state = np.where(inside, LIT, OUT_OF_CONE).astype(np.int8)
            if light["castShadow"]:
                facing = (normal * to_light).sum(-1) > 0
                state[inside & ~facing] = FACING_AWAY
                ask = np.flatnonzero(inside & facing)
                if ask.size:
                    blocked = np.isfinite(self.trace(pos[ask], to_light[ask])[0])
                    state[ask[blocked]] = SHADOWED
            states[:, li] = state
            if li != drop_light:
                total += np.where(state == LIT, lambert, 0.0)
        colour = self.colour(inst_idx, tri, bary)
        return states, np.minimum(1.0, np.maximum(0.2, total)[:, None] * colour)


def render_view(scene, view, lights, res, drop_light=None, decide=True):
    """depth [res,res] f64, rgb [res,res,4] u8, decided [res,res] bool, the
    centre rays' per-light states [res,res,L] and instance [res,res] (-1 on a
    miss) for one view."""
    view = np.ascontiguousarray(view).view(VIEW_DT).ravel()[0]
    lights = np.ascontiguousarray(lights).view(LIGHT_DT).ravel()
    offsets = [(0.0, 0.0)]
    if decide:
        offsets += [(DELTA, DELTA), (DELTA, -DELTA), (-DELTA, DELTA), (-DELTA, -DELTA)]
    outcome = []
    for k, (du, dv) in enumerate(offsets):
        start, d = view_rays(view, res, du, dv)
        d = d.reshape(-1, 3)
        org = np.broadcast_to(start, d.shape).copy()
        t, inst, tri, bary = scene.trace(org, d) if len(scene.inst) else (
            np.full(len(d), np.inf), np.full(len(d), -1), np.full(len(d), -1),
            np.zeros((len(d), 2)))
        hit = np.isfinite(t)
        states = -np.ones((len(d), len(lights)), np.int8)
        shaded = np.zeros((len(d), 3))
        if hit.any():
            states[hit], shaded[hit] = scene.shade(org[hit], d[hit], t[hit], inst[hit],
                                                   tri[hit], bary[hit], lights, drop_light)
        outcome.append((hit, inst, tri, states))
        if k == 0:
            depth = np.where(hit, t, 0.0).reshape(res, res)
            rgb = np.zeros((res * res, 4), np.uint8)
            rgb[:, :3] = np.floor(shaded * 255.0).astype(np.uint8)
            rgb[:, 3] = 255
            centre_states = states.reshape(res, res, -1)
            centre_inst = np.where(hit, inst, -1).reshape(res, res)
    decided = np.ones(res * res, bool)
    hit0, inst0, tri0, states0 = outcome[0]
    for hit, inst, tri, states in outcome[1:]:
        decided &= (hit == hit0) & (inst == inst0) & (tri == tri0) & \
            (states == states0).all(-1)
    return depth, rgb.reshape(res, res, 4), decided.reshape(res, res), centre_states, \
        centre_inst


def split_rows(rows, counts):
    at = np.concatenate([[0], np.cumsum(counts)])
    return [rows[at[w]:at[w + 1]] for w in range(len(counts))]


def render_worlds(geo, instances, inst_counts, views, lights, light_counts, res,
                  worlds=None, drop_light=None, decide=True):
    """Every view (two per world, world-major) of the given worlds.  Returns
    depth [V,res,res], rgb [V,res,res,4], decided [V,res,res], a list of the
    per-view light states and the hit instances [V,res,res] (index in the
    world's rows as given)."""
    inst = split_rows(np.ascontiguousarray(instances).view(INSTANCE_DT).ravel(), inst_counts)
    lit = split_rows(np.ascontiguousarray(lights).view(LIGHT_DT).ravel(), light_counts)
    views = np.ascontiguousarray(views).view(VIEW_DT).ravel()
    worlds = range(len(inst_counts)) if worlds is None else worlds
    depth, rgb, decided, states, hit_inst = [], [], [], [], []
    for w in worlds:
        scene = Scene(geo, inst[w])
        mine = views[views["worldIDX"] == w]
        assert len(mine) == 2, (w, len(mine))
        for v in mine:
            a, b, c, s, i = render_view(scene, v, lit[w], res, drop_light, decide)
            depth.append(a), rgb.append(b), decided.append(c), states.append(s)
            hit_inst.append(i)
    return np.stack(depth), np.stack(rgb), np.stack(decided), states, np.stack(hit_inst)
