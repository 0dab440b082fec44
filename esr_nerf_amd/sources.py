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

Everything up to the file is device tensors; nothing here copies the mesh to the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from . import mesh

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
           "source_samples", "source_visibility", "VERTEX_PROPERTIES"]
