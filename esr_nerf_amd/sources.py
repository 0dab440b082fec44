"""The product of a run as geometry: the extracted surface with normals, materials and emission per vertex, and the list
of its emissive sources as connected surface patches.

The reference hands its user a bare ``trimesh.Trimesh(vertices, triangles)`` (app/fine/pdra.py:781, lts.py:659,
fine.py:632) and knows emissive sources only per view, as the image masks ``any(lin/emit > k_val)`` (pdra.py:686-688,
911).  Here the same criterion is applied on the surface:

``extract_surface``    mesh.sdf_field + mesh.marching_cubes (the smoothed field, as ``extract_geometry``), vertices moved to
                       world space on the device, ``ESRNeRF.surface_attributes`` at the vertices (the raw grids)
``emissive_sources``   a vertex is emissive iff max_c emission > k_val; a face is selected iff its three vertices are;
                       the sources are the connected components of the selected faces (mesh.connected_components: two
                       faces are connected iff they share a vertex) with mesh.component_stats of each
``simplify_surface``   mesh.simplify / mesh.simplify_to on a Surface: fewer, larger faces with the attributes re-queried
                       from the model or area-weighted from the old vertices, and the faces' source ids carried along
``write_surface_ply``  a binary PLY with the attributes per vertex and the source id per face (chamfer.read_ply reads the
                       mesh back)

``source_lights``      the sources as area-weighted point lights at ``source_samples``' points, with edits applied
``direct_light``       their light at surface points, shadowed by the surface, reflected once by the light-transport stage's
                       Disney BRDF or as irradiance: one fused launch (csrc/surflight.hip, header section U)
``lit_view``           the same for the pixels of a camera view, with the environment's light on request
``environment_light``  the light of the spherical-Gaussian environment map at surface points over a table of hemisphere
                       directions (``hemisphere_directions``), shadowed by the surface, with one more bounce from a vertex
                       radiance (``vertex_env_radiance``): one fused launch (csrc/surfenv.hip, header section V)

``bake_materials``     the materials at the texel centres of a texture atlas (``atlas.build``; csrc/atlas.hip, header section
                       W): queried from the model at every owned texel's point, or interpolated from the vertices
``bake_irradiance``    ``direct_light`` per source and ``environment_light`` as irradiance at the texels inside their faces
``write_surface_obj``  OBJ + MTL with the baked maps as 8-bit PNGs (emission also as Radiance .hdr and .npy)

Everything up to the file is device tensors; nothing here copies the mesh to the host.
"""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, mesh

ATTR_KEYS = ("normal", "sdf", "basecolor", "roughness", "metallic", "emission")


@dataclass
class Surface:
    vertices: torch.Tensor               # device float64 [V, 3], world space
    triangles: torch.Tensor              # device int64 [F, 3]; (b - a) x (c - a) points outward
    attrs: Dict[str, torch.Tensor]       # device float32: normal [V,3], sdf [V], basecolor [V,3], roughness [V], metallic [V],
                                         # emission [V,3]


@dataclass
class SourceReport:
    k_val: float
    face_source: torch.Tensor            # device int32 [F]: the source of each face, -1 for a face in none
    n_faces: torch.Tensor                # int64 [S]
    area: torch.Tensor                   # float64 [S]
    centroid: torch.Tensor               # float64 [S, 3]: area-weighted
    bbox_min: torch.Tensor               # float64 [S, 3]
    bbox_max: torch.Tensor               # float64 [S, 3]
    mean_emission: torch.Tensor          # float64 [S, 3]: area-weighted
    peak_emission: torch.Tensor          # float32 [S]: the largest emission channel at a vertex of the source
    area_centroid: torch.Tensor          # float64 [S, 3]: the raw sum of area * face centre (centroid * area)
    area_emission: torch.Tensor          # float64 [S, 3]: the raw sum of area * face-mean emission (mean_emission * area)

    def __len__(self):
        return int(self.n_faces.shape[0])


@torch.no_grad()
def extract_surface(model, resolution=512, threshold=0.0, smooth: bool = True, sigma: float = 0.5, chunk: int = 1 << 18) -> Surface:
    """The zero level set of the model's SDF with what the model knows at every vertex.  The geometry comes from the
    smoothed field, exactly as ``mesh.extract_geometry`` builds it (v / (R - 1) * (max - min) + min, in float64); the
    attributes come from the raw grids (``ESRNeRF.surface_attributes``)."""
    u = mesh.sdf_field(model, resolution, smooth, sigma)
    verts, tris = mesh.marching_cubes(u, threshold)
    dev = verts.device
    lo, hi = (b.to(dev) for b in mesh._box(model))
    res = torch.tensor(u.shape, dtype=torch.float64, device=dev)
    # (the extent is a float32 difference, as in extract_geometry: the same bits as its numpy expression)
    world = verts / (res - 1.0)[None, :] * (hi - lo).double()[None, :] + lo.double()[None, :]
    # a vertex on the face of the box may round past it in float32: the attributes are those of the box's face
    pts = torch.minimum(torch.maximum(world.float(), lo), hi)
    attrs = model.surface_attributes(pts, chunk=chunk)
    return Surface(world.contiguous(), tris, {k: attrs[k] for k in ATTR_KEYS})


@torch.no_grad()
def emissive_sources(surface: Surface, k_val: float, min_area: float = 0.0) -> SourceReport:
    """The emissive sources of a surface as connected patches: PDRA's criterion ``any(emission > k_val)`` per vertex, the
    faces whose three vertices pass it, their connected components (shared vertex) and the sums over each.  Sources with
    an area under ``min_area`` are dropped: their faces get -1 and the others keep their order."""
    v, t = surface.vertices, surface.triangles
    em = surface.attrs["emission"].contiguous()
    hot = em.max(dim=1).values > float(k_val)
    sel = hot[t].all(dim=1) if t.shape[0] else torch.zeros(0, dtype=torch.bool, device=t.device)
    label, k = mesh.connected_components(t, v.shape[0], sel)
    st = mesh.component_stats(v, t, label, k, em)
    if min_area > 0.0 and k:
        keep = st["area"] >= float(min_area)
        renum = (torch.cumsum(keep.to(torch.int32), 0) - 1).to(torch.int32)
        renum[~keep] = -1
        label = torch.where(label >= 0, renum[label.clamp_min(0).long()], label)
        st = {name: x[keep] for name, x in st.items()}
    return SourceReport(float(k_val), label, st["n_faces"], st["area"], st["centroid"], st["bbox_min"], st["bbox_max"],
                        st["mean_attr"], st["peak"], st["area_centroid"], st["area_attr"])


_ATTR_WIDTH = {"normal": 3, "sdf": 1, "basecolor": 3, "roughness": 1, "metallic": 1, "emission": 3}


@torch.no_grad()
def simplify_surface(surface: Surface, cell: Optional[float] = None, target_faces: Optional[int] = None, model=None,
                     face_source: Optional[torch.Tensor] = None, lam: float = 1e-3, chunk: int = 1 << 18):
    """The surface simplified by quadric vertex clustering: ``mesh.simplify`` at the cell size ``cell`` (world units) or
    ``mesh.simplify_to`` at ``target_faces``; exactly one of the two is given.  -> ``(Surface, face_source')``.

    With ``model`` the attributes are queried again at the new vertices (``surface_attributes``, the points clamped to
    the model's box as ``extract_surface`` clamps them).  Without it they are the area-weighted means of the old
    vertices' (the 12 channels of ``ATTR_KEYS`` go through the kernel together) and the normals are normalised again.
    ``face_source`` (int32 [F], ``SourceReport.face_source``) is carried to the kept faces: ``face_source[face_origin]``;
    None stays None.  The result is a Surface like any other: ``emissive_sources``, ``write_surface_ply``,
    ``raster.rasterize`` and ``raster.edit_view_data`` take it unchanged."""
    if (cell is None) == (target_faces is None):
        raise ValueError("simplify_surface: give exactly one of cell and target_faces")
    v, t = surface.vertices, surface.triangles
    if face_source is not None and (not isinstance(face_source, torch.Tensor) or face_source.shape != (t.shape[0],) or
                                    face_source.device != t.device):
        raise ValueError("simplify_surface: face_source must have one entry per face, on the surface's device")
    packed = None
    if model is None:
        packed = torch.cat([surface.attrs[k].reshape(v.shape[0], -1).float() for k in ATTR_KEYS], dim=1).contiguous()
    if cell is not None:
        nv, nt, na, _, face_origin = mesh.simplify(v, t, cell, lam=lam, attr=packed)
    else:
        (nv, nt, na, _, face_origin), _, _ = mesh.simplify_to(v, t, target_faces, lam=lam, attr=packed)
    if model is None:
        attrs, at = {}, 0
        for k in ATTR_KEYS:
            w = _ATTR_WIDTH[k]
            attrs[k] = na[:, at:at + w].reshape((-1, 3) if surface.attrs[k].dim() == 2 else (-1,)).contiguous()
            at += w
        attrs["normal"] = torch.nn.functional.normalize(attrs["normal"], dim=1)
    else:
        lo, hi = (b.to(nv.device) for b in mesh._box(model))
        got = model.surface_attributes(torch.minimum(torch.maximum(nv.float(), lo), hi), chunk=chunk)
        attrs = {k: got[k] for k in ATTR_KEYS}
    return Surface(nv.contiguous(), nt.contiguous(), attrs), None if face_source is None else face_source[face_origin]


VISIBILITY_CHUNK = 1 << 22               # most segments of one launch of source_visibility


def source_samples(surface: Surface, report: SourceReport, samples: int = 16):
    """The sample points of every source, fixed by the mesh alone: a source's faces in id order, their cumulative area in
    float64 (area = 0.5 sqrt((n0 n0 + n1 n1) + n2 n2), n = (b - a) x (c - a)); sample k of n = min(samples, n_faces) is
    the centre ((a + b) + c) * (1 / 3) of the first face whose cumulative area reaches (k + 1/2) / n of the total.
    -> (face int32 [S, samples], point float64 [S, samples, 3], n int64 [S]); the slots k >= n of a source are unused."""
    samples = int(samples)
    if samples < 1:
        raise ValueError(f"source_samples: samples must be at least 1, got {samples}")
    v, t, fs = surface.vertices, surface.triangles, report.face_source
    dev, S = v.device, len(report)
    if S == 0 or t.shape[0] == 0:
        return (torch.zeros(S, samples, dtype=torch.int32, device=dev), torch.zeros(S, samples, 3, dtype=torch.float64, device=dev),
                torch.zeros(S, dtype=torch.int64, device=dev))
    key = torch.where(fs < 0, S, fs.long())
    skey, order = torch.sort(key, stable=True)
    a, b, c = (v[t[order, k]] for k in range(3))
    e1, e2 = b - a, c - a
    # (every product and difference is its own launch: nothing can be contracted into an fma)
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = torch.sqrt((n0 * n0 + n1 * n1) + n2 * n2) * 0.5
    area = torch.where(torch.isfinite(area), area, torch.zeros_like(area))
    cum = torch.cumsum(area, 0)
    start = torch.searchsorted(skey, torch.arange(S + 1, dtype=torch.int64, device=dev))
    zero = torch.zeros(1, dtype=torch.float64, device=dev)
    edge = torch.cat([zero, cum])[start]                              # the cumulative area before each source's first face
    base, total = edge[:-1], edge[1:] - edge[:-1]
    count = start[1:] - start[:-1]
    n = count.clamp(max=samples)
    k = torch.arange(samples, dtype=torch.float64, device=dev)
    thr = base[:, None] + ((k[None, :] + 0.5) / n.clamp(min=1).double()[:, None]) * total[:, None]
    j = torch.searchsorted(cum, thr.contiguous())
    j = torch.minimum(torch.maximum(j, start[:-1, None]), (start[1:, None] - 1).clamp(min=0))
    point = ((a[j] + b[j]) + c[j]) * (1.0 / 3.0)                     # (a product: a device division by a number is not one rounding)
    return order[j].to(torch.int32), point, n


@torch.no_grad()
def source_visibility(surface: Surface, report: SourceReport, points: torch.Tensor, samples: int = 16, bvh=None,
                      eps: float = 1e-6) -> torch.Tensor:
    """float32 [P, S]: for every query point and every source of ``report`` the share of the source's sample points
    (``source_samples``) the point sees.  A sample is seen iff no face other than the sample's own is hit strictly inside
    the segment from the point to the sample (``raycast.occluded_segments`` with ``skip_face``).  All P * S * n segments go
    through the any-hit walk, at most ``VISIBILITY_CHUNK`` per launch; the mean is taken on the device and nothing is read
    back.  ``bvh``: the ``raycast.Bvh`` of the surface, built here when None."""
    from . import raycast
    v = surface.vertices
    dev, S = v.device, len(report)
    if not isinstance(points, torch.Tensor) or points.device != dev or points.dim() != 2 or points.shape[1] != 3 or \
            points.dtype not in (torch.float32, torch.float64):
        raise ValueError("source_visibility: points must be a float [P, 3] tensor on the surface's device")
    P = int(points.shape[0])
    out = torch.zeros(P, S, dtype=torch.float32, device=dev)
    if P == 0 or S == 0:
        return out
    if bvh is None:
        bvh = raycast.build(v, surface.triangles)
    face, point, n = source_samples(surface, report, samples)
    K = face.shape[1]
    valid = torch.arange(K, device=dev)[None, :] < n[:, None]           # [S, K]
    pts = points.double()
    step = max(1, VISIBILITY_CHUNK // (S * K))
    for p0 in range(0, P, step):
        p = pts[p0:p0 + step]
        m = int(p.shape[0])
        occ = raycast.occluded_segments(bvh, p[:, None, None, :].expand(m, S, K, 3).reshape(-1, 3),
                                        point[None].expand(m, S, K, 3).reshape(-1, 3),
                                        skip_face=face[None].expand(m, S, K).reshape(-1), eps=eps).reshape(m, S, K)
        seen = ((occ == 0) & valid[None]).sum(-1)
        out[p0:p0 + step] = (seen.double() / n.clamp(min=1).double()[None, :]).float()
    return out


MAX_LIGHT_SLOTS = _lib.SURFACE_LIGHT_MAX_SLOTS   # a source's sample slots sit in one wave


@dataclass
class SourceLights:
    """The sources of a surface as point lights, slot-major as ``esr_surface_light`` takes them: Kp slots per source (a power
    of two), of which the first ``n[s]`` are used"""
    point: torch.Tensor                  # device float64 [S, Kp, 3]: the sample points (face centres)
    normal: torch.Tensor                 # device float64 [S, Kp, 3]: the unit normal of the sample's face
    weight: torch.Tensor                 # device float64 [S, Kp]: area_s / n_s, the area a sample stands for; 0 in an unused slot
    radiance: torch.Tensor               # device float32 [S, Kp, 3]: the mean emission of the face's vertices, edited
    face: torch.Tensor                   # device int32 [S, Kp]: the sample's face (the shadow segment never hits it)
    n: torch.Tensor                      # device int64 [S]: the used slots of every source

    def __len__(self):
        return int(self.point.shape[0])

    @property
    def slots(self) -> int:
        return int(self.point.shape[1])


def _edit_tables(what, n_sources, edits, dev):
    """per source: (mode int64 [S], intensity float32 [S], colour float32 [S, 2]) of ``raster.edit_view_data``'s edit dicts;
    a source in no edit is unchanged.  Refuses before anything is launched."""
    from .raster import EDIT_MODES, _conditions
    from .relight import LIGHT_MODES
    modes, inten, cols = [LIGHT_MODES["on"]] * n_sources, [1.0] * n_sources, [[0.0, 0.0] for _ in range(n_sources)]
    groups = []
    for e in edits:
        if not isinstance(e, dict) or e.get("mode") not in EDIT_MODES:
            raise ValueError(f"{what}: an edit is a dict whose mode is one of {EDIT_MODES}")
        col = [float(c) for c in e.get("color", (0.0, 0.0, 0.0))]
        if len(col) not in (2, 3):
            raise ValueError(f"{what}: a colour has 2 or 3 components, got {len(col)}")
        groups.append(list(e.get("sources", ())))
    try:
        cond = _conditions(n_sources, groups)
    except ValueError as err:
        raise ValueError(f"{what}: {err}") from None
    for s in range(n_sources):
        if cond[s] >= 0:
            e = edits[int(cond[s])]
            modes[s], inten[s] = LIGHT_MODES[e["mode"]], float(e.get("intensity", 1.0))
            cols[s] = [float(c) for c in e.get("color", (0.0, 0.0, 0.0))][:2]
    return (torch.tensor(modes, dtype=torch.int64).reshape(n_sources).to(dev),
            torch.tensor(inten, dtype=torch.float32).reshape(n_sources).to(dev),
            torch.tensor(cols, dtype=torch.float32).reshape(n_sources, 2).to(dev))


@torch.no_grad()
def source_lights(surface: Surface, report: SourceReport, samples: int = 16, edits=None) -> SourceLights:
    """The sources of ``report`` as the point lights of ``direct_light``: the sample points and faces of ``source_samples``;
    per sample the unit normal n / |n|, n = (b - a) x (c - a), of its face (float64, every operation its own launch, as in
    ``source_samples``), the weight ``area_s / n_s`` (the area one sample stands for) and the radiance ((e_a + e_b) + e_c) *
    (1 / 3) of the face's three vertex emissions (float32).  ``Kp``, the slots per source, is the next power of two >=
    ``samples`` (at most 64 samples); the slots from ``n_s`` on have weight 0 and are never used.
    ``edits``: the dicts of ``raster.edit_view_data`` (``sources``, ``mode``, ``intensity``, ``color``: hue and saturation
    first), applied to every sample of their sources through ``relight.edit_emission``.  No read-back."""
    samples = int(samples)
    if samples < 1 or samples > MAX_LIGHT_SLOTS:
        raise ValueError(f"source_lights: 1 .. {MAX_LIGHT_SLOTS} samples per source, got {samples}")
    S, dev = len(report), surface.vertices.device
    tables = _edit_tables("source_lights", S, edits, dev) if edits else None
    kp = 1
    while kp < samples:
        kp *= 2
    face, point, n = source_samples(surface, report, samples)
    v, t = surface.vertices, surface.triangles
    f = face.long()
    if t.shape[0]:
        a, b, c = (v[t[f, k]] for k in range(3))                          # [S, samples, 3]
        em = surface.attrs["emission"].float()
        ea, eb, ec = (em[t[f, k]] for k in range(3))
    else:
        a = b = c = torch.zeros(S, samples, 3, dtype=torch.float64, device=dev)
        ea = eb = ec = torch.zeros(S, samples, 3, dtype=torch.float32, device=dev)
    e1, e2 = b - a, c - a
    n0 = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
    n1 = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
    n2 = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
    length = torch.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    normal = torch.stack([n0, n1, n2], -1) / length[..., None]
    radiance = ((ea + eb) + ec) * (1.0 / 3.0)
    used = torch.arange(samples, device=dev)[None, :] < n[:, None]       # [S, samples]
    weight = (report.area.double() / n.clamp(min=1).double())[:, None].expand(S, samples)
    if tables is not None and S:
        from .relight import edit_emission
        modes, inten, cols = (x[:, None].expand(S, samples, *x.shape[1:]).reshape(S * samples, *x.shape[1:]).contiguous()
                              for x in tables)
        radiance = edit_emission(radiance.reshape(-1, 3), modes, inten, cols).reshape(S, samples, 3)

    def slots(x, fill):
        out = torch.full((S, kp) + tuple(x.shape[2:]), fill, dtype=x.dtype, device=dev)
        out[:, :samples] = torch.where(used.reshape(S, samples, *([1] * (x.dim() - 2))), x, torch.full_like(x, fill))
        return out.contiguous()
    return SourceLights(slots(point, 0.0), slots(normal, 0.0), slots(weight, 0.0), slots(radiance, 0.0), slots(face, -1), n)


def _light_input(what, name, x, shape, dev, dtypes=(torch.float32, torch.float64)):
    if not isinstance(x, torch.Tensor) or x.device != dev or x.dtype not in dtypes or tuple(x.shape) != shape:
        raise ValueError(f"{what}: {name} must be a float {list(shape)} tensor on the surface's device")
    return x


@torch.no_grad()
def direct_light(surface: Surface, lights: SourceLights, points: torch.Tensor, normals: torch.Tensor, basecolor=None,
                 roughness=None, metallic=None, wo=None, bvh=None, per_source: bool = False, eps: float = 1e-6,
                 return_seen: bool = False):
    """The light of the sources ``lights`` (``source_lights``) at the surface points ``points`` [P, 3] with the unit shading
    normals ``normals`` [P, 3], shadowed by the surface, in one fused launch (``esr_surface_light``, section U of
    include/esr_hip.h): per point, source and sample the geometric term ``G = cos_l A / max(r^2, A)`` in float64, the shadow
    segment of ``raycast.occluded_segments`` (``eps``, the sample's own face skipped) only where G is not zero, and

    with ``wo`` [P, 3] (unit, towards the viewer), ``basecolor`` [P, 3], ``roughness`` [P] and ``metallic`` [P]: the radiance
    reflected towards ``wo`` by the Disney BRDF of the light-transport stage (the model's ``emo`` component, one bounce);
    with ``wo=None``: the irradiance, sum of cos_x G E (no BRDF, no view).

    -> float32 [P, 3], the sum over the sources (in float64, in source order, rounded once), or with ``per_source`` the
    kernel's [P, S, 3]: an intensity edit of a source is a re-weighting of that.  ``return_seen`` adds uint8 [P, S, Kp]: 0 a
    sample that contributes nothing unshadowed (unused, behind the point or the source facing away), 1 seen, 2 shadowed.

    A sample is a point light standing for the area A = area_s / n_s; the clamp max(r^2, A) keeps it bounded, so within
    about one sample spacing of a source the estimate is LOW (far from it, it converges on the area integral).  ``bvh``: the
    ``raycast.Bvh`` of the surface, built here when None.  The same input gives the same bytes on every call; no read-back."""
    from . import raycast
    what = "direct_light"
    v = surface.vertices
    dev = v.device
    if not isinstance(lights, SourceLights):
        raise ValueError(f"{what}: lights is a SourceLights (source_lights)")
    S, kp = len(lights), lights.slots
    if kp < 1 or kp > MAX_LIGHT_SLOTS or kp & (kp - 1):
        raise ValueError(f"{what}: {kp} slots per source; a power of two up to {MAX_LIGHT_SLOTS}")
    for name, x, shape, dt in (("point", lights.point, (S, kp, 3), torch.float64), ("normal", lights.normal, (S, kp, 3), torch.float64),
                               ("weight", lights.weight, (S, kp), torch.float64), ("radiance", lights.radiance, (S, kp, 3), torch.float32),
                               ("face", lights.face, (S, kp), torch.int32)):
        if not isinstance(x, torch.Tensor) or x.device != dev or x.dtype != dt or tuple(x.shape) != shape:
            raise ValueError(f"{what}: lights.{name} must be a {dt} {list(shape)} tensor on the surface's device")
    if not isinstance(points, torch.Tensor) or points.dim() != 2:
        raise ValueError(f"{what}: points must be a float [P, 3] tensor on the surface's device")
    P = int(points.shape[0])
    _light_input(what, "points", points, (P, 3), dev)
    _light_input(what, "normals", normals, (P, 3), dev)
    if P >= 2 ** 31 or S >= 2 ** 31:
        raise ValueError(f"{what}: {P} points and {S} sources exceed the kernel's 31-bit counts")
    if not 0.0 <= float(eps) < 0.5:
        raise ValueError(f"{what}: eps is in [0, 0.5), got {eps}")
    mode = 1 if wo is None else 0
    mat = [None] * 4
    if mode == 0:
        if basecolor is None or roughness is None or metallic is None:
            raise ValueError(f"{what}: with wo the reflection needs basecolor, roughness and metallic")
        mat = [_light_input(what, name, x, shape, dev).float().contiguous()
               for name, x, shape in (("basecolor", basecolor, (P, 3)), ("roughness", roughness, (P,)), ("metallic", metallic, (P,)),
                                      ("wo", wo, (P, 3)))]
    if bvh is None:
        bvh = raycast.build(v, surface.triangles)
    elif not isinstance(bvh, raycast.Bvh) or bvh.vertices.device != dev:
        raise ValueError(f"{what}: bvh is the raycast.Bvh of the surface")
    out = torch.zeros(P, S, 3, dtype=torch.float32, device=dev)
    seen = torch.zeros(P, S, kp, dtype=torch.uint8, device=dev) if return_seen else None
    if P and S:
        pts, nrm = points.double().contiguous(), normals.float().contiguous()
        arrays = [x.contiguous() for x in (lights.point, lights.normal, lights.weight, lights.radiance, lights.face)]
        args = _lib.EsrSurfaceLight(
            nodes=_lib.ptr(bvh.nodes), n_faces=bvh.n_faces, vertices=_lib.ptr(bvh.vertices), n_vertices=int(bvh.vertices.shape[0]),
            triangles=_lib.ptr(bvh.triangles), n_sources=S, slots=kp, mode=mode,
            l_point=_lib.ptr(arrays[0]), l_normal=_lib.ptr(arrays[1]), l_weight=_lib.ptr(arrays[2]), l_radiance=_lib.ptr(arrays[3]),
            l_face=_lib.ptr(arrays[4]), n_points=P, p_point=_lib.ptr(pts), p_normal=_lib.ptr(nrm), p_base=_lib.ptr(mat[0]),
            p_rough=_lib.ptr(mat[1]), p_metal=_lib.ptr(mat[2]), p_wo=_lib.ptr(mat[3]), eps=float(eps), out=_lib.ptr(out),
            seen=_lib.ptr(seen))
        import ctypes
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().esr_surface_light(ctypes.byref(args), _lib.stream_ptr(dev)), "esr_surface_light")
    if not per_source:
        total = torch.zeros(P, 3, dtype=torch.float64, device=dev)
        for s in range(S):                                                # (source order: the same bytes whatever torch's sum does)
            total = total + out[:, s].double()
        out = total.float()
    return (out, seen) if return_seen else out


MAX_ENV_DIRS = _lib.SURFACE_ENV_MAX_DIRS
MAX_ENV_SG = _lib.SURFACE_ENV_MAX_SG


def hemisphere_directions(n: int, device=None) -> torch.Tensor:
    """float32 [n, 3]: the reference's ``fibonacci_spiral_samples_on_unit_hemisphere(n)`` (app/utils/pbr/functions.py:176-194
    with ``random=False, up=True``), restated operation by operation on the host -- the upper half (z > 0) of a Fibonacci
    spiral of 2 n points -- and copied to ``device``.  The mean of its z is exactly 1/2."""
    n = int(n)
    if n < 1 or n > MAX_ENV_DIRS:
        raise ValueError(f"hemisphere_directions: 1 .. {MAX_ENV_DIRS} directions, got {n}")
    m = 2 * n
    rn = torch.arange(n, m)
    ga = np.pi * (3.0 - np.sqrt(5.0))
    phi = ga * ((rn + 1.0) % m)
    cos_theta = ((rn + 0.5) * (1.0 / n)) - 1.0
    sin_theta = torch.sqrt(1.0 - cos_theta * cos_theta)
    out = torch.stack([torch.cos(phi) * sin_theta, torch.sin(phi) * sin_theta, cos_theta], dim=-1)
    return out if device is None else out.to(device)


def _env_parameters(what, env, dev):
    """(mus [J, 3], lambdas [J], lobes [J, 3]) float32 on ``dev`` of a SphericalGaussian or of a (mus, lambdas, lobes) tuple"""
    if isinstance(env, (tuple, list)):
        if len(env) != 3:
            raise ValueError(f"{what}: env is a SphericalGaussian or a (mus, lambdas, lobes) tuple")
        mus, lambdas, lobes = env
    elif all(hasattr(env, k) for k in ("mus", "lambdas", "lobes")):
        mus, lambdas, lobes = env.mus, env.lambdas, env.lobes
    else:
        raise ValueError(f"{what}: env is a SphericalGaussian or a (mus, lambdas, lobes) tuple")
    for name, x in (("mus", mus), ("lambdas", lambdas), ("lobes", lobes)):
        if not isinstance(x, torch.Tensor) or x.device != dev or x.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{what}: env.{name} must be a float tensor on the surface's device")
    J = int(mus.shape[0]) if mus.dim() == 2 else -1
    if J < 1 or J > MAX_ENV_SG or tuple(mus.shape) != (J, 3) or tuple(lobes.shape) != (J, 3) or lambdas.numel() != J:
        raise ValueError(f"{what}: env holds 1 .. {MAX_ENV_SG} lobes: mus [J, 3], lambdas [J] or [J, 1], lobes [J, 3]")
    return tuple(x.detach().float().contiguous() for x in (mus, lambdas.reshape(J), lobes))


def _env_dirs(what, dirs, dev):
    if isinstance(dirs, torch.Tensor):
        R = int(dirs.shape[0]) if dirs.dim() == 2 else -1
        if dirs.device != dev or dirs.dtype not in (torch.float32, torch.float64) or R < 1 or tuple(dirs.shape) != (R, 3):
            raise ValueError(f"{what}: dirs is a count or a float [R, 3] tensor of unit directions on the surface's device")
        if R > MAX_ENV_DIRS:
            raise ValueError(f"{what}: at most {MAX_ENV_DIRS} directions, got {R}")
        return dirs.float().contiguous()
    if isinstance(dirs, bool) or not isinstance(dirs, int) or not 1 <= dirs <= MAX_ENV_DIRS:
        raise ValueError(f"{what}: dirs is a count in 1 .. {MAX_ENV_DIRS} or a float [R, 3] tensor, got {dirs!r}")
    return hemisphere_directions(dirs, dev)


@torch.no_grad()
def environment_light(surface: Surface, env, points: torch.Tensor, normals: torch.Tensor, basecolor=None, roughness=None,
                      metallic=None, wo=None, dirs=128, faces=None, vertex_radiance=None, bvh=None, t_min: float = 1e-6,
                      return_open: bool = False, return_hit: bool = False):
    """The light of the environment map ``env`` at the surface points ``points`` [P, 3] with the unit shading normals
    ``normals`` [P, 3], in one fused launch (``esr_surface_env``, section V of include/esr_hip.h): per point the R directions
    of one table (``dirs``: a count, then ``hemisphere_directions``, or a float [R, 3] tensor) are flipped into the normal's
    hemisphere as the reference's ``diffuse_scattering_fib`` flips them, cast against the surface from ``t_min`` on (the face
    ``faces`` [P] int32 of each point never hit; -1: none), and the incoming radiance -- the environment where the ray leaves
    the mesh; where it hits, 0 or with ``vertex_radiance`` float32 [V, 3] that radiance interpolated on the nearest face -- is

    with ``wo`` [P, 3] (unit, towards the viewer), ``basecolor`` [P, 3], ``roughness`` [P] and ``metallic`` [P]: reflected
    towards ``wo`` by the Disney BRDF of the light-transport stage, the mean over the directions (the reference's
    ``lin/env_dir``, with ``vertex_radiance`` plus its ``lin/env_indir``);
    with ``wo=None``: the irradiance, 2 pi times the mean of L cos.

    ``env`` is the model's ``SphericalGaussian`` or a ``(mus, lambdas, lobes)`` tuple of its raw parameters: an environment
    is edited by passing rotated lobes or scaled mus.  -> float32 [P, 3]; ``return_open`` adds float32 [P], the share of
    directions that leave the mesh (n_open / R); ``return_hit`` adds uint8 [P, R].  ``bvh``: the ``raycast.Bvh`` of the
    surface, built here when None.  One table of directions serves all points.  The same input gives the same bytes on every
    call; no read-back."""
    from . import raycast
    what = "environment_light"
    v = surface.vertices
    dev = v.device
    mus, lambdas, lobes = _env_parameters(what, env, dev)
    table = _env_dirs(what, dirs, dev)
    R = int(table.shape[0])
    if not isinstance(points, torch.Tensor) or points.dim() != 2:
        raise ValueError(f"{what}: points must be a float [P, 3] tensor on the surface's device")
    P = int(points.shape[0])
    _light_input(what, "points", points, (P, 3), dev)
    _light_input(what, "normals", normals, (P, 3), dev)
    if P >= 2 ** 31:
        raise ValueError(f"{what}: {P} points exceed the kernel's 31-bit count")
    if not float(t_min) >= 0.0:
        raise ValueError(f"{what}: t_min is not negative, got {t_min}")
    if faces is not None:
        _light_input(what, "faces", faces, (P,), dev, dtypes=(torch.int32,))
    V = int(v.shape[0])
    if vertex_radiance is not None:
        _light_input(what, "vertex_radiance", vertex_radiance, (V, 3), dev)
    mode = 1 if wo is None else 0
    mat = [None] * 4
    if mode == 0:
        if basecolor is None or roughness is None or metallic is None:
            raise ValueError(f"{what}: with wo the reflection needs basecolor, roughness and metallic")
        mat = [_light_input(what, name, x, shape, dev).float().contiguous()
               for name, x, shape in (("basecolor", basecolor, (P, 3)), ("roughness", roughness, (P,)), ("metallic", metallic, (P,)),
                                      ("wo", wo, (P, 3)))]
    if bvh is None:
        bvh = raycast.build(v, surface.triangles)
    elif not isinstance(bvh, raycast.Bvh) or bvh.vertices.device != dev:
        raise ValueError(f"{what}: bvh is the raycast.Bvh of the surface")
    out = torch.zeros(P, 3, dtype=torch.float32, device=dev)
    n_open = torch.zeros(P, dtype=torch.int32, device=dev) if return_open else None
    hit = torch.zeros(P, R, dtype=torch.uint8, device=dev) if return_hit else None
    if P:
        pts, nrm = points.double().contiguous(), normals.float().contiguous()
        rad = None if vertex_radiance is None else vertex_radiance.float().contiguous()
        fc = None if faces is None else faces.contiguous()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().esr_surface_env(
                _lib.ptr(bvh.nodes), bvh.n_faces, _lib.ptr(bvh.vertices), int(bvh.vertices.shape[0]), _lib.ptr(bvh.triangles),
                _lib.ptr(table), R, _lib.ptr(mus), _lib.ptr(lambdas), _lib.ptr(lobes), int(mus.shape[0]), _lib.ptr(rad), P,
                _lib.ptr(pts), _lib.ptr(nrm), _lib.ptr(fc), _lib.ptr(mat[0]), _lib.ptr(mat[1]), _lib.ptr(mat[2]), _lib.ptr(mat[3]),
                mode, float(t_min), _lib.ptr(out), _lib.ptr(n_open), _lib.ptr(hit), _lib.stream_ptr(dev)), "esr_surface_env")
    res = (out,)
    if return_open:
        res += (n_open.float() / float(R),)
    if return_hit:
        res += (hit,)
    return res if len(res) > 1 else out


@torch.no_grad()
def vertex_env_radiance(surface: Surface, env, dirs=128, bvh=None) -> torch.Tensor:
    """float32 [V, 3]: ``environment_light`` at every vertex with the vertex's own normal (normalised again) and material and
    ``wo`` = that normal -- the view-independent first bounce of the environment's light, for baking and as the
    ``vertex_radiance`` of a second gather."""
    a = surface.attrs
    n = a["normal"].float()
    n = n / torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).clamp(min=1e-12)[:, None]
    return environment_light(surface, env, surface.vertices, n, a["basecolor"].float().reshape(-1, 3), a["roughness"].float().reshape(-1),
                             a["metallic"].float().reshape(-1), n, dirs=dirs, bvh=bvh)


MAX_PATHS = _lib.SURFACE_PATH_MAX_PATHS
MAX_PATH_DEPTH = _lib.SURFACE_PATH_MAX_DEPTH
PATH_CHUNK = 1 << 20                     # most points of one launch of path_light


@torch.no_grad()
def path_light(surface: Surface, report: SourceReport, points: torch.Tensor, normals: torch.Tensor, faces=None, basecolor=None,
               roughness=None, metallic=None, wo=None, env=None, paths: int = 64, depth: int = 2, samples: int = 16, edits=None,
               seed: int = 0, mode: int = 0, bvh=None, chunk: int = PATH_CHUNK, t_min: float = 1e-6, eps: float = 1e-6,
               return_trace: bool = False, lights=None, sampling: str = "uniform", roulette=None):
    """Path-traced light at the surface points ``points`` [P, 3] with the unit shading normals ``normals`` [P, 3]
    (``esr_surface_path``, section X of include/esr_hip.h): ``paths`` paths per point of up to ``depth`` segments.  Every
    segment takes a uniform random direction in the hemisphere of its vertex's normal (the light-transport stage's
    ``diffuse_scattering``; Philox4x32-10 keyed by ``seed``, the counter names point, path and segment) and weights the path by
    the Disney reflection there; a segment that leaves the mesh collects the environment ``env`` (as ``environment_light`` takes
    it; None: no environment) and ends the path; at every vertex a segment reaches, one random sample of every source of
    ``report`` (``source_lights(surface, report, samples, edits)``, or ``lights`` where the caller holds them already) is gathered
    with ``direct_light``'s term and shadow segment.

    ``mode`` 0: the radiance reflected towards ``wo`` [P, 3] by ``basecolor`` [P, 3], ``roughness`` [P], ``metallic`` [P];
    ``mode`` 1: the irradiance at the point (the first vertex weighs by cos 2 pi instead; no material, no ``wo``).
    ``faces`` int32 [P]: the face each point lies on, which its first segment never hits (-1: none).  The vertices a path
    reaches take the surface's per-vertex normal, basecolor, roughness and metallic, interpolated.

    -> dict of float32 [P, 3] ``env_dir`` (the environment seen directly from the point), ``env_indir`` (the environment by way
    of other surface points), ``src_indir`` (the sources by way of other surface points; their direct light is
    ``direct_light``'s) and float32 [P] ``open``, the share of first segments that leave the mesh.  ``return_trace`` adds
    ``trace`` int32 [P, paths, depth] (the face each segment hit, -1 where it left the mesh, -2 where it was not cast) and
    ``end`` uint8 [P, paths] (0 the depth is used up, 1 left the mesh, 2 reached a back face).

    ``sampling`` "brdf" (``esr_surface_path_is``, section Y) draws every segment's direction from the vertex's BRDF instead: a
    cosine-distributed direction or the specular lobe's half vector, chosen by the material and weighted by one-sample multiple
    importance sampling -- the same expectation at far less noise, with other random numbers and so other bytes than
    "uniform".  There ``roulette=k`` (an integer >= 1) starts Russian roulette at segment ``k``: a path goes on with the
    probability max(throughput) clamped to [1/16, 1] and is weighted by its inverse; None: no roulette.  ``end`` then also holds
    3 (ended by the roulette) and 4 (the draw left the hemisphere: no light comes from there).  ``roulette`` with "uniform" is
    refused.

    Points beyond ``chunk`` go in several launches that give the bytes of one.  Limits: the sources are point samples with
    ``direct_light``'s near-field clamp, no sampling inside faces; with the default ``sampling`` a fixed depth without Russian
    roulette and without importance sampling of the BRDF.  The same input gives the same bytes on every call; nothing is read
    back."""
    import ctypes
    from . import raycast
    what = "path_light"
    v = surface.vertices
    dev = v.device
    for name, x, lo, hi in (("paths", paths, 1, MAX_PATHS), ("depth", depth, 1, MAX_PATH_DEPTH), ("mode", mode, 0, 1)):
        if isinstance(x, bool) or not isinstance(x, int) or not lo <= x <= hi:
            raise ValueError(f"{what}: {name} is an integer in {lo} .. {hi}, got {x!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{what}: seed is an integer in 0 .. 2^64 - 1, got {seed!r}")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"{what}: chunk is a positive count of points, got {chunk!r}")
    rr_start = _path_sampling(what, sampling, roulette, depth)
    samples = int(samples)
    if samples < 1 or samples > MAX_LIGHT_SLOTS:
        raise ValueError(f"{what}: 1 .. {MAX_LIGHT_SLOTS} samples per source, got {samples}")
    if not float(t_min) >= 0.0:
        raise ValueError(f"{what}: t_min is not negative, got {t_min}")
    if not 0.0 <= float(eps) < 0.5:
        raise ValueError(f"{what}: eps is in [0, 0.5), got {eps}")
    sg = [None, None, None] if env is None else _env_parameters(what, env, dev)
    if not isinstance(points, torch.Tensor) or points.dim() != 2:
        raise ValueError(f"{what}: points must be a float [P, 3] tensor on the surface's device")
    P = int(points.shape[0])
    _light_input(what, "points", points, (P, 3), dev)
    _light_input(what, "normals", normals, (P, 3), dev)
    if P >= 2 ** 31:
        raise ValueError(f"{what}: {P} points exceed the kernel's 31-bit count")
    if faces is not None:
        _light_input(what, "faces", faces, (P,), dev, dtypes=(torch.int32,))
    mat = [None] * 4
    if mode == 0:
        if basecolor is None or roughness is None or metallic is None or wo is None:
            raise ValueError(f"{what}: mode 0 needs basecolor, roughness, metallic and wo")
        mat = [_light_input(what, name, x, shape, dev).float().contiguous()
               for name, x, shape in (("basecolor", basecolor, (P, 3)), ("roughness", roughness, (P,)), ("metallic", metallic, (P,)),
                                      ("wo", wo, (P, 3)))]
    V = int(v.shape[0])
    attrs = []
    for key, width in (("normal", 3), ("basecolor", 3), ("roughness", 1), ("metallic", 1)):
        x = surface.attrs.get(key)
        if not isinstance(x, torch.Tensor) or x.device != dev or x.numel() != V * width:
            raise ValueError(f"{what}: the surface carries no per-vertex {key}")
        attrs.append(x.float().reshape(V, width).contiguous())
    if bvh is None:
        bvh = raycast.build(v, surface.triangles)
    elif not isinstance(bvh, raycast.Bvh) or bvh.vertices.device != dev:
        raise ValueError(f"{what}: bvh is the raycast.Bvh of the surface")
    if lights is None:
        lights = source_lights(surface, report, samples, edits)
    elif not isinstance(lights, SourceLights) or lights.point.device != dev:
        raise ValueError(f"{what}: lights is the SourceLights of source_lights on the surface's device")
    S, kp = len(lights), lights.slots
    out = torch.zeros(P, 3, 3, dtype=torch.float32, device=dev)
    n_open = torch.zeros(P, dtype=torch.int32, device=dev)
    trace = torch.zeros(P, paths, depth, dtype=torch.int32, device=dev) if return_trace else None
    end = torch.zeros(P, paths, dtype=torch.uint8, device=dev) if return_trace else None
    if P:
        pts, nrm = points.double().contiguous(), normals.float().contiguous()
        fc = None if faces is None else faces.contiguous()
        arrays = [x.contiguous() for x in (lights.point, lights.normal, lights.weight, lights.radiance, lights.face)]
        signed = seed - 2 ** 64 if seed >= 2 ** 63 else seed               # (the 64 bits, as the int64 the entry takes)
        cut = lambda x, a, b: None if x is None else _lib.ptr(x[a:b])
        entry = "esr_surface_path" if rr_start is None else "esr_surface_path_is"
        controls = (mode, paths, depth) if rr_start is None else (mode, paths, depth, rr_start)
        with torch.cuda.device(dev):
            for p0 in range(0, P, chunk):
                p1 = min(P, p0 + chunk)
                _lib.check(getattr(_lib.lib(), entry)(
                    _lib.ptr(bvh.nodes), bvh.n_faces, _lib.ptr(bvh.vertices), int(bvh.vertices.shape[0]), _lib.ptr(bvh.triangles),
                    _lib.ptr(attrs[0]), _lib.ptr(attrs[1]), _lib.ptr(attrs[2]), _lib.ptr(attrs[3]), S, kp, _lib.ptr(arrays[0]),
                    _lib.ptr(arrays[1]), _lib.ptr(arrays[2]), _lib.ptr(arrays[3]), _lib.ptr(arrays[4]), float(eps), _lib.ptr(sg[0]),
                    _lib.ptr(sg[1]), _lib.ptr(sg[2]), 0 if env is None else int(sg[0].shape[0]), p1 - p0, cut(pts, p0, p1),
                    cut(nrm, p0, p1), cut(fc, p0, p1), cut(mat[0], p0, p1), cut(mat[1], p0, p1), cut(mat[2], p0, p1),
                    cut(mat[3], p0, p1), *controls, float(t_min), signed, p0, cut(out, p0, p1), cut(n_open, p0, p1),
                    cut(trace, p0, p1), cut(end, p0, p1), _lib.stream_ptr(dev)), entry)
    res = {"env_dir": out[:, 0], "env_indir": out[:, 1], "src_indir": out[:, 2], "open": n_open.float() / float(paths)}
    if return_trace:
        res["trace"], res["end"] = trace, end
    return res


def _path_sampling(what, sampling, roulette, depth):
    """-> None for "uniform" (section X), else section Y's ``rr_start``: ``roulette``, or ``depth`` (no roulette) for None"""
    if sampling not in ("uniform", "brdf"):
        raise ValueError(f'{what}: sampling is "uniform" or "brdf", got {sampling!r}')
    if roulette is not None:
        if sampling == "uniform":
            raise ValueError(f'{what}: roulette comes with sampling="brdf"')
        if isinstance(roulette, bool) or not isinstance(roulette, int) or not 1 <= roulette < 2 ** 31:
            raise ValueError(f"{what}: roulette is the first segment it runs at, an integer >= 1, or None; got {roulette!r}")
    return None if sampling == "uniform" else (depth if roulette is None else roulette)


def _hit_points(surface: Surface, hit, d):
    """What ``lit_view`` knows at the nearest hits ``hit`` (``raycast.Hits``) of the rays with the directions ``d``: the point
    (float64, NaN where the ray misses: such a point is lit by nothing), the unit shading normal, the interpolated
    attributes and ``wo``.  The barycentric weights are (1 - u) - v, u, v; every operation is its own launch."""
    v, t = surface.vertices, surface.triangles
    tri = t[hit.face.clamp(min=0).long()]                                  # [N, 3]
    bu, bv = hit.bary[:, 0], hit.bary[:, 1]
    b64 = torch.stack([(1.0 - bu) - bv, bu, bv], 1)                        # the weights of the face's three vertices
    b32 = b64.float()

    def at(x, b):
        x = x.reshape(x.shape[0], -1)
        return (x[tri[:, 0]] * b[:, 0:1] + x[tri[:, 1]] * b[:, 1:2]) + x[tri[:, 2]] * b[:, 2:3]

    def unit(x):
        return x / torch.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]).clamp(min=1e-12)[:, None]
    nan = torch.full((1, 3), float("nan"), dtype=torch.float64, device=v.device)
    x = torch.where((hit.face >= 0)[:, None], at(v, b64), nan)
    a = {k: at(surface.attrs[k].float(), b32) for k in ("normal", "basecolor", "roughness", "metallic", "emission")}
    return x, unit(a["normal"]), a, (-unit(d)).float()


@torch.no_grad()
def lit_view(surface: Surface, report: SourceReport, cams, view: int, samples: int = 16, edits=None, bvh=None, env=None,
             env_dirs=128, bounces: int = 0, atlas=None, textures=None, paths=None, depth: int = 2, seed: int = 0,
             sampling: str = "uniform", roulette=None):
    """View ``view`` of ``cams`` lit by the (edited) sources, without an optimiser step: the nearest face of every pixel
    (the rays and the walk of ``raycast.cast_cameras``), the vertex attributes interpolated with the hit's barycentrics in
    torch (the normal normalised again), ``wo`` = minus the unit pixel ray, and ``direct_light`` with ``source_lights(surface,
    report, samples, edits)``.  -> dict of

    ``lin/reflect`` float32 [H, W, 3]  the sources' light reflected once towards the camera (the model's ``emo`` component)
    ``lin/emit``    float32 [H, W, 3]  the interpolated emission, edited, where the pixel's face belongs to a source
    ``face``        int32 [H, W]       as ``cast_cameras``; -1 where the ray misses
    ``depth``       float64 [H, W]     as ``cast_cameras``; +inf where the ray misses

    With ``env`` (the model's ``SphericalGaussian`` or a ``(mus, lambdas, lobes)`` tuple, as ``environment_light`` takes it)
    the light of the environment is added, over the ``env_dirs`` hemisphere directions (a count or a [R, 3] table):

    ``lin/env_dir``   float32 [H, W, 3]  the environment's light that reaches the pixel's point directly, reflected towards
                                         the camera (the reference's ``lin/env_dir`` on the surface)
    ``etc/open``      float32 [H, W]     the share of the point's directions that leave the mesh
    ``lin/env_indir`` float32 [H, W, 3]  only with ``bounces == 1``: the environment's light that reaches the point by way of
                                         one other surface point -- a second launch whose rays take ``vertex_env_radiance``
                                         from the face they hit, minus ``lin/env_dir``

    With ``env=None`` the keys and their bytes are those above and nothing else.  A pixel that misses is 0 in every image.
    The linear image of the edited scene is ``lin/emit + lin/reflect + lin/env_dir (+ lin/env_indir)``.  Limits: one table
    of directions for all points (no per-point random rotation), one extra bounce at the most, and that bounce is
    view-independent (the radiance a vertex sends along its own normal stands for every direction).  The near-field limit of
    ``direct_light`` applies.  Nothing is read back.

    With ``atlas`` and ``textures`` (``atlas.build`` of this surface and the dict of ``bake_materials``; both or neither) the
    basecolor, roughness, metallic, emission and the shading normal of every pixel are looked up in the textures
    (``atlas.sample`` at the hit's face and barycentrics; the normal normalised again) instead of interpolated from the
    vertices; ``face`` and ``depth`` are unchanged.  With None the keys and bytes are those of the vertex path.

    With ``paths`` (a count; ``depth`` segments, ``seed``) the light beyond the first reflection is path-traced
    (``path_light`` with the pixel's point as the first vertex): ``lin/env_dir``, ``lin/env_indir`` and ``etc/open`` come from
    the paths (``env`` may be None: they are 0 then), ``env_dirs`` is unused, ``bounces`` must be left at 0, and

    ``lin/src_indir`` float32 [H, W, 3]  the sources' light that reaches the pixel's point by way of other surface points

    is added; the linear image is ``lin/emit + lin/reflect + lin/src_indir + lin/env_dir + lin/env_indir``.  ``atlas`` and
    ``textures`` affect the first vertex only: the vertices a path reaches take the per-vertex attributes.  ``sampling`` and
    ``roulette`` are ``path_light``'s ("brdf": directions drawn from the BRDF, the same keys at far less noise; they need
    ``paths``).  With ``paths=None`` the keys and bytes are exactly those described above."""
    from . import raycast
    from .relight import edit_emission
    what = "lit_view"
    if (atlas is None) != (textures is None):
        raise ValueError(f"{what}: atlas and textures come together")
    if textures is not None and any(k not in textures for k in TEXTURE_KEYS):
        raise ValueError(f"{what}: textures holds {TEXTURE_KEYS}")
    if isinstance(view, bool) or not isinstance(view, int) or not 0 <= view < cams.n_views:
        raise ValueError(f"{what}: view {view!r} of a set of {cams.n_views}")
    samples = int(samples)
    if samples < 1 or samples > MAX_LIGHT_SLOTS:
        raise ValueError(f"{what}: 1 .. {MAX_LIGHT_SLOTS} samples per source, got {samples}")
    v, t = surface.vertices, surface.triangles
    dev, S = v.device, len(report)
    if cams.device != dev:
        raise ValueError(f"{what}: the surface and the cameras are on one device")
    tables = _edit_tables(what, S, edits, dev) if edits else None
    if paths is not None:
        if isinstance(bounces, bool) or bounces != 0:
            raise ValueError(f"{what}: with paths the bounces are the paths': bounces stays 0, got {bounces!r}")
        for name, x, lo, hi in (("paths", paths, 1, MAX_PATHS), ("depth", depth, 1, MAX_PATH_DEPTH)):
            if isinstance(x, bool) or not isinstance(x, int) or not lo <= x <= hi:
                raise ValueError(f"{what}: {name} is an integer in {lo} .. {hi}, got {x!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"{what}: seed is an integer in 0 .. 2^64 - 1, got {seed!r}")
        _path_sampling(what, sampling, roulette, depth)
        if env is not None:
            env = _env_parameters(what, env, dev)
    elif sampling != "uniform" or roulette is not None:
        raise ValueError(f"{what}: sampling and roulette are the paths': they need paths")
    elif env is not None:
        if isinstance(bounces, bool) or bounces not in (0, 1):
            raise ValueError(f"{what}: bounces is 0 or 1, got {bounces!r}")
        env = _env_parameters(what, env, dev)
        env_dirs = _env_dirs(what, env_dirs, dev)
    if bvh is None:
        bvh = raycast.build(v, t)
    lights = source_lights(surface, report, samples, edits)
    H, W = cams.height, cams.width
    o, d, _ = raycast.pixel_rays(cams, view)
    hit = raycast.cast(bvh, o, d)
    if not t.shape[0]:                                                     # (no face: every ray misses)
        black = torch.zeros(H, W, 3, dtype=torch.float32, device=dev)
        res = {"lin/reflect": black, "lin/emit": black.clone(), "face": hit.face.reshape(H, W), "depth": hit.t.reshape(H, W)}
        if paths is not None:
            res["lin/env_dir"], res["lin/env_indir"], res["lin/src_indir"] = black.clone(), black.clone(), black.clone()
            res["etc/open"] = torch.zeros(H, W, dtype=torch.float32, device=dev)
        elif env is not None:
            res["lin/env_dir"], res["etc/open"] = black.clone(), torch.zeros(H, W, dtype=torch.float32, device=dev)
            if bounces:
                res["lin/env_indir"] = black.clone()
        return res
    got = hit.face >= 0
    x, normal, a, wo = _hit_points(surface, hit, d)
    if atlas is not None:
        normal, a = _hit_textures(what, surface, atlas, textures, hit)
    reflect = direct_light(surface, lights, x, normal, a["basecolor"], a["roughness"][:, 0], a["metallic"][:, 0], wo, bvh=bvh)
    src = report.face_source[hit.face.clamp(min=0).long()]
    lit = got & (src >= 0)
    emit = a["emission"].contiguous()
    if tables is not None and S:
        sid = src.clamp(min=0).long()
        emit = edit_emission(emit, tables[0][sid].contiguous(), tables[1][sid].contiguous(), tables[2][sid].contiguous())
    zero = torch.zeros(1, 3, dtype=torch.float32, device=dev)
    res = {"lin/reflect": torch.where(got[:, None], reflect, zero).reshape(H, W, 3),
           "lin/emit": torch.where(lit[:, None], emit, zero).reshape(H, W, 3),
           "face": hit.face.reshape(H, W), "depth": hit.t.reshape(H, W)}
    if paths is not None:
        lit_by = path_light(surface, report, x, normal, hit.face, a["basecolor"], a["roughness"][:, 0], a["metallic"][:, 0], wo, env=env,
                            paths=paths, depth=depth, samples=samples, edits=edits, seed=seed, bvh=bvh, lights=lights, sampling=sampling,
                            roulette=roulette)
        for k in ("env_dir", "env_indir", "src_indir"):
            res["lin/" + k] = torch.where(got[:, None], lit_by[k], zero).reshape(H, W, 3)
        res["etc/open"] = torch.where(got, lit_by["open"], zero[0, 0]).reshape(H, W)
    elif env is not None:
        at = (x, normal, a["basecolor"], a["roughness"][:, 0], a["metallic"][:, 0], wo)
        direct, share = environment_light(surface, env, *at, dirs=env_dirs, faces=hit.face, bvh=bvh, return_open=True)
        res["lin/env_dir"] = torch.where(got[:, None], direct, zero).reshape(H, W, 3)
        res["etc/open"] = torch.where(got, share, zero[0, 0]).reshape(H, W)
        if bounces:
            both = environment_light(surface, env, *at, dirs=env_dirs, faces=hit.face, bvh=bvh,
                                     vertex_radiance=vertex_env_radiance(surface, env, env_dirs, bvh=bvh))
            res["lin/env_indir"] = torch.where(got[:, None], both - direct, zero).reshape(H, W, 3)
    return res


TEXTURE_KEYS = ("normal", "basecolor", "roughness", "metallic", "emission")


def _hit_textures(what, surface, atlas, textures, hit):
    """the unit shading normal and the material dict of ``_hit_points`` from the textures: one ``atlas.sample`` of the 11
    channels at the hits"""
    from . import atlas as _atlas
    if int(atlas.uv.shape[0]) != int(surface.triangles.shape[0]):
        raise ValueError(f"{what}: the atlas was built from another surface")
    W = atlas.size
    packed = torch.cat([textures[k].float().reshape(W, W, -1) for k in TEXTURE_KEYS], dim=2).contiguous()
    got = _atlas.sample(atlas, packed, hit.face, hit.bary)
    a, at = {}, 0
    for k in TEXTURE_KEYS:
        a[k] = got[:, at:at + _ATTR_WIDTH[k]].contiguous()
        at += _ATTR_WIDTH[k]
    n = a["normal"]
    n = n / torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).clamp(min=1e-12)[:, None]
    return n, a


def _check_atlas(what, surface, atlas):
    from .atlas import Atlas
    if not isinstance(atlas, Atlas) or atlas.face is None or atlas.face.device != surface.vertices.device or \
            int(atlas.uv.shape[0]) != int(surface.triangles.shape[0]):
        raise ValueError(f"{what}: atlas is the atlas.build of this surface")


@torch.no_grad()
def bake_materials(surface: Surface, atlas, model=None, chunk: int = 1 << 18) -> Dict[str, torch.Tensor]:
    """The materials at the texel centres of ``atlas`` (``atlas.build(surface.vertices, surface.triangles, ...)``) -> dict of
    device float32 textures for ``ATTR_KEYS``: ``normal``, ``basecolor``, ``emission`` [W, W, 3], ``sdf``, ``roughness``,
    ``metallic`` [W, W]; 0 where a texel belongs to no face.

    With ``model``: ``surface_attributes`` at the world point of every owned texel (gutter texels included: their points lie
    on the face's plane just outside it), the points clamped to the model's box as ``extract_surface`` clamps them.  The
    detail is the model's, not the mesh's.  Without: the vertex attributes interpolated (in the gutter, extrapolated) by the
    texel pass itself, all 12 channels in one launch; normals are not normalised again (``lit_view`` does that per pixel)."""
    from . import atlas as _atlas
    what = "bake_materials"
    _check_atlas(what, surface, atlas)
    W, dev = atlas.size, surface.vertices.device
    if model is None:
        packed = torch.cat([surface.attrs[k].reshape(surface.vertices.shape[0], -1).float() for k in ATTR_KEYS], dim=1).contiguous()
        tex = _atlas.texels(atlas, surface.vertices, surface.triangles, packed)[4]
        out, at = {}, 0
        for k in ATTR_KEYS:
            w = _ATTR_WIDTH[k]
            out[k] = (tex[:, :, at:at + w] if surface.attrs[k].dim() == 2 else tex[:, :, at]).contiguous()
            at += w
        return out
    own = (atlas.face >= 0).reshape(-1)
    idx = torch.nonzero(own).reshape(-1)
    lo, hi = (b.to(dev) for b in mesh._box(model))
    pts = torch.minimum(torch.maximum(atlas.point.reshape(-1, 3)[idx], lo), hi)
    got = model.surface_attributes(pts, chunk=chunk) if idx.numel() else None
    out = {}
    for k in ATTR_KEYS:
        w = _ATTR_WIDTH[k]
        flat = torch.zeros(W * W, w, dtype=torch.float32, device=dev)
        if got is not None:
            flat[idx] = got[k].reshape(-1, w).float()
        out[k] = flat.reshape(W, W, w) if k in ("normal", "basecolor", "emission") else flat.reshape(W, W)
    return out


@torch.no_grad()
def bake_irradiance(surface: Surface, atlas, report: SourceReport, samples: int = 16, edits=None, env=None, env_dirs=128, bvh=None,
                    chunk: int = 1 << 18, paths=None, depth: int = 2, seed: int = 0, roulette=None) -> Dict[str, torch.Tensor]:
    """The irradiance at the texels of ``atlas`` whose centre lies inside their face, with the face's geometric unit normal:

    ``light/sources`` float32 [W, W, S, 3]  ``direct_light(per_source=True)`` without ``wo``: per source, so that an intensity
                                            edit stays a re-weighting of the texture
    ``light/env``     float32 [W, W, 3]     only with ``env``: ``environment_light`` without ``wo`` over ``env_dirs``, the
                                            texel's own face skipped as ``lit_view`` skips the hit face

    ``light/paths``   float32 [W, W, 3, 3]  only with ``paths`` (a count; ``depth`` segments, ``seed``, ``roulette``): the
                                            path-traced irradiance, ``path_light(mode=1, sampling="brdf")`` -- its components
                                            env_dir, env_indir, src_indir in this order, the texel's own face skipped by the
                                            first segment; ``env`` may be None (the two environment components are 0 then)

    0 at every other texel.  ``chunk`` texels per launch (the paths' bytes do not depend on it)."""
    from . import raycast
    what = "bake_irradiance"
    _check_atlas(what, surface, atlas)
    if paths is not None:
        for name, x, lo, hi in (("paths", paths, 1, MAX_PATHS), ("depth", depth, 1, MAX_PATH_DEPTH)):
            if isinstance(x, bool) or not isinstance(x, int) or not lo <= x <= hi:
                raise ValueError(f"{what}: {name} is an integer in {lo} .. {hi}, got {x!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"{what}: seed is an integer in 0 .. 2^64 - 1, got {seed!r}")
        _path_sampling(what, "brdf", roulette, depth)
    elif roulette is not None:
        raise ValueError(f"{what}: roulette is the paths': it needs paths")
    v, t = surface.vertices, surface.triangles
    W, dev, S = atlas.size, v.device, len(report)
    if bvh is None:
        bvh = raycast.build(v, t)
    lights = source_lights(surface, report, samples, edits)
    if env is not None:
        env = _env_parameters(what, env, dev)
        env_dirs = _env_dirs(what, env_dirs, dev)
    idx = torch.nonzero(((atlas.flags & 1) != 0).reshape(-1)).reshape(-1)
    face = atlas.face.reshape(-1)[idx].contiguous()
    pts = atlas.point.reshape(-1, 3)[idx].double()
    nrm = face_normals(surface)[face.long()]
    src = torch.zeros(W * W, S, 3, dtype=torch.float32, device=dev)
    out = {"light/sources": src}
    if env is not None:
        out["light/env"] = torch.zeros(W * W, 3, dtype=torch.float32, device=dev)
    step = max(1, int(chunk))
    for c0 in range(0, int(idx.shape[0]), step):
        sl = slice(c0, c0 + step)
        src[idx[sl]] = direct_light(surface, lights, pts[sl], nrm[sl], bvh=bvh, per_source=True)
        if env is not None:
            out["light/env"][idx[sl]] = environment_light(surface, env, pts[sl], nrm[sl], dirs=env_dirs, faces=face[sl].contiguous(),
                                                          bvh=bvh)
    out["light/sources"] = src.reshape(W, W, S, 3)
    if env is not None:
        out["light/env"] = out["light/env"].reshape(W, W, 3)
    if paths is not None:
        lit = path_light(surface, report, pts, nrm, face.contiguous(), env=env, paths=paths, depth=depth, samples=samples, edits=edits,
                         seed=seed, mode=1, bvh=bvh, chunk=step, lights=lights, sampling="brdf", roulette=roulette)
        traced = torch.zeros(W * W, 3, 3, dtype=torch.float32, device=dev)
        traced[idx] = torch.stack([lit["env_dir"], lit["env_indir"], lit["src_indir"]], 1)
        out["light/paths"] = traced.reshape(W, W, 3, 3)
    return out


def face_normals(surface: Surface) -> torch.Tensor:
    """float32 [F, 3]: the unit normal n / |n|, n = (b - a) x (c - a), of every face (float64, every operation its own launch,
    as ``source_lights``; a degenerate face gets 0)"""
    v, t = surface.vertices, surface.triangles
    a, b, c = (v[t[:, k]] for k in range(3))
    e1, e2 = b - a, c - a
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    length = torch.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    n = torch.stack([n0, n1, n2], -1) / length[:, None]
    return torch.where(torch.isfinite(n).all(dim=1, keepdim=True), n, torch.zeros_like(n)).float()


def quantise8(x: np.ndarray) -> np.ndarray:
    """uint8: x clamped to [0, 1] (NaN -> 0), times 255, rounded half to even"""
    x = np.nan_to_num(np.asarray(x, dtype=np.float64), nan=0.0)
    return np.rint(np.clip(x, 0.0, 1.0) * 255.0).astype(np.uint8)


def png_bytes(image: np.ndarray) -> bytes:
    """an 8-bit PNG (grey for [H, W] or [H, W, 1], RGB for [H, W, 3]) of a uint8 array: zlib and struct, no imaging package;
    filter 0 on every row"""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3)) or img.size == 0:
        raise ValueError("png_bytes: a uint8 [H, W], [H, W, 1] or [H, W, 3] array")
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * c)], axis=1)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)
    head = struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", head) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b"")


def hdr_bytes(image: np.ndarray) -> bytes:
    """a flat (not run-length encoded) Radiance RGBE picture of a float [H, W, 3] array; negative and NaN values are 0"""
    img = np.nan_to_num(np.asarray(image, dtype=np.float64), nan=0.0, posinf=3e38)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("hdr_bytes: a float [H, W, 3] array")
    img = np.clip(img, 0.0, None)
    h, w = img.shape[:2]
    top = img.max(axis=2)
    mant, expo = np.frexp(top)                                          # top = mant 2^expo, mant in [0.5, 1)
    live = top > 1e-32
    scale = np.where(live, np.ldexp(1.0, 8 - expo), 0.0)                 # 256 / 2^expo
    px = np.zeros((h, w, 4), np.uint8)
    px[..., :3] = np.minimum(np.floor(img * scale[..., None]), 255).astype(np.uint8)
    px[..., 3] = np.where(live, np.clip(expo + 128, 0, 255), 0).astype(np.uint8)
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode("ascii") + px.tobytes()


def write_surface_obj(path, surface: Surface, atlas, textures, gamma=None):
    """The surface as ``path`` (an .obj) with its baked maps beside it -> the list of the files written.

    OBJ: ``v`` (repr of the float64 coordinates), three ``vt`` per face (u = x / W, v = 1 - y / W: image row 0 is the top)
    and ``f v/vt``, 1-based.  MTL (same stem): ``map_Kd`` basecolor, ``map_Pr`` roughness, ``map_Pm`` metallic, ``map_Ke``
    emission, ``norm`` the normal as n / 2 + 1 / 2.  The maps are 8-bit PNGs (``png_bytes``), clamped to [0, 1] and rounded
    half to even; basecolor goes through ``gamma`` first (default ``metrics.apply_gamma_curve``), the others are linear.
    Emission exceeds 1, so it is also written as a flat Radiance ``_emission.hdr`` and as ``_emission.npy`` (float32)."""
    _need = [k for k in TEXTURE_KEYS if k not in textures]
    if _need:
        raise ValueError(f"write_surface_obj: textures lacks {_need}")
    W = atlas.size
    stem = os.path.splitext(str(path))[0]
    name = os.path.basename(stem)
    v = np.asarray(surface.vertices.detach().cpu(), dtype=np.float64).reshape(-1, 3)
    t = np.asarray(surface.triangles.detach().cpu(), dtype=np.int64).reshape(-1, 3)
    uv = np.asarray(atlas.uv.detach().cpu(), dtype=np.float64).reshape(-1, 2)
    if len(uv) != 3 * len(t):
        raise ValueError("write_surface_obj: the atlas was built from another surface")
    if gamma is None:
        from .metrics import apply_gamma_curve as gamma
    host = lambda x: np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    tex = {k: host(textures[k]).reshape(W, W, -1) for k in TEXTURE_KEYS}
    maps = {"basecolor": host(gamma(textures["basecolor"])).reshape(W, W, 3), "roughness": tex["roughness"], "metallic": tex["metallic"],
            "emission": tex["emission"], "normal": tex["normal"] * np.float32(0.5) + np.float32(0.5)}
    files = [stem + ".obj", stem + ".mtl"]
    lines = [f"mtllib {name}.mtl", "usemtl surface"]
    lines += [f"v {x!r} {y!r} {z!r}" for x, y, z in v.tolist()]
    lines += [f"vt {a!r} {1.0 - b!r}" for a, b in uv.tolist()]
    lines += [f"f {a + 1}/{3 * f + 1} {b + 1}/{3 * f + 2} {c + 1}/{3 * f + 3}" for f, (a, b, c) in enumerate(t.tolist())]
    with open(files[0], "w") as f:
        f.write("\n".join(lines) + "\n")
    keys = (("map_Kd", "basecolor"), ("map_Pr", "roughness"), ("map_Pm", "metallic"), ("map_Ke", "emission"), ("norm", "normal"))
    with open(files[1], "w") as f:
        f.write("newmtl surface\nKd 1 1 1\nKe 1 1 1\n" + "".join(f"{key} {name}_{k}.png\n" for key, k in keys))
    for _, k in keys:
        files.append(f"{stem}_{k}.png")
        with open(files[-1], "wb") as f:
            f.write(png_bytes(quantise8(maps[k])))
    files.append(stem + "_emission.hdr")
    with open(files[-1], "wb") as f:
        f.write(hdr_bytes(tex["emission"]))
    files.append(stem + "_emission.npy")
    np.save(files[-1], tex["emission"])
    return files


VERTEX_PROPERTIES = ["x", "y", "z", "nx", "ny", "nz", "basecolor_r", "basecolor_g", "basecolor_b", "roughness", "metallic",
                     "emission_r", "emission_g", "emission_b"]


def write_surface_ply(path, surface: Surface, face_source: Optional[torch.Tensor] = None):
    """A binary little-endian PLY of the surface: per vertex ``double x y z`` then ``float nx ny nz basecolor_r/g/b
    roughness metallic emission_r/g/b``; per face ``list uchar int vertex_indices`` and, with ``face_source``, ``int
    source``.  ``chamfer.read_ply`` reads vertices and faces back unchanged (it skips the other properties)."""
    a = {k: np.asarray(x.detach().cpu()) for k, x in surface.attrs.items()}
    v = np.asarray(surface.vertices.detach().cpu(), dtype=np.float64).reshape(-1, 3)
    t = np.asarray(surface.triangles.detach().cpu(), dtype=np.int64).reshape(-1, 3)
    vrec = np.empty(len(v), dtype=[(p, "<f8" if p in VERTEX_PROPERTIES[:3] else "<f4") for p in VERTEX_PROPERTIES])
    cols = np.concatenate([a["normal"].reshape(-1, 3), a["basecolor"].reshape(-1, 3), a["roughness"].reshape(-1, 1),
                           a["metallic"].reshape(-1, 1), a["emission"].reshape(-1, 3)], axis=1)
    for i, p in enumerate("xyz"):
        vrec[p] = v[:, i]
    for i, p in enumerate(VERTEX_PROPERTIES[3:]):
        vrec[p] = cols[:, i]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {'double' if p in VERTEX_PROPERTIES[:3] else 'float'} {p}" for p in VERTEX_PROPERTIES]
    head += [f"element face {len(t)}", "property list uchar int vertex_indices"]
    fdt = [("n", "u1"), ("v", "<i4", (3,))]
    if face_source is not None:
        head.append("property int source")
        fdt.append(("source", "<i4"))
    head.append("end_header")
    frec = np.empty(len(t), dtype=fdt)
    frec["n"] = 3
    frec["v"] = t
    if face_source is not None:
        src = np.asarray(face_source.detach().cpu() if isinstance(face_source, torch.Tensor) else face_source)
        if src.shape != (len(t),):
            raise ValueError("write_surface_ply: face_source must have one entry per face")
        frec["source"] = src
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


__all__ = ["Surface", "SourceReport", "extract_surface", "emissive_sources", "simplify_surface", "write_surface_ply",
           "source_samples", "source_visibility", "SourceLights", "source_lights", "direct_light", "lit_view", "VERTEX_PROPERTIES",
           "hemisphere_directions", "environment_light", "vertex_env_radiance", "TEXTURE_KEYS", "bake_materials", "bake_irradiance",
           "face_normals", "write_surface_obj", "png_bytes", "hdr_bytes", "quantise8"]
