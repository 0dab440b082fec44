"""Write tests/golden/surface_points.npz: the reference's own per-point surface attributes at seeded points.

    python tools/gen_surface_golden.py            (CPU host with the reference tree)

The reference ``ESRNeRF`` is imported at run time through the stubs of oracle/ref_import.py, built on the g16 slab scene
with the parameters of tests/golden/lts_g16_params.npz and put in eval mode (``emit_color`` is ``emo_color`` there,
esrnerf.py:237-238).  At 257 seeded points inside the bounding box (257 is no multiple of the 32-point tile) it runs the
reference's own lines: ``sample_sdf_grad`` (the SDF value), ``sample_sdf_expgrad`` (the gradient; the normal is its
``F.normalize``), ``sample_sdfeat_grad_normal`` and the positional encoding (the features of esrnerf.py:1341-1348),
``brdf`` / ``emit_color`` and ``brdfnet`` / ``emitnet`` (esrnerf.py:1124-1137).

Only data goes into the file: the points, the six outputs, a threshold ``k_val`` and the 257 decisions
``max_c emission > k_val``.  ``k_val`` is the midpoint of the widest gap between consecutive sorted per-point emission
maxima in the middle half of the points; the tool asserts that this gap is at least 4e-4 max|emission|, so that no
result within the project's parity bar (1e-4 of the largest value, either way) can flip a decision.

The emission head of these parameters (small random weights, zero last bias) stays within a few percent of softplus(0)
over the whole box, so 257 uniform draws leave no such gap (the widest of twelve seeds: 2.7e-4 of 0.71).  The points
are therefore the first 257 of a seeded pool of 1024 uniform draws whose reference emission maximum lies further than
2.5e-4 max|emission| from the pool's median: chosen on the reference's values alone, before any kernel of this
project runs.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("ESR_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")
N_POINTS = 257
N_POOL = 1024
SEED = 31
CLEAR = 2.5e-4             # half-width of the band around the pool's median that holds no point, in max|emission|


def seeded_pool(lo, hi):
    """1024 float32 points inside the box, a twentieth of its extent away from every face"""
    rng = np.random.default_rng(SEED)
    u = 0.05 + 0.9 * rng.random((N_POOL, 3))
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + u * (hi - lo)).astype(np.float32)


def pick_k_val(emission):
    """(k_val, gap): the midpoint and the width of the widest gap between consecutive sorted per-point maxima in the
    middle half of the points"""
    m = np.sort(emission.max(1).astype(np.float64))
    n = len(m)
    a, b = n // 4, n - n // 4
    gaps = np.diff(m[a:b])
    i = int(np.argmax(gaps))
    return np.float32((m[a + i] + m[a + i + 1]) / 2), float(gaps[i])


def generate():
    from esr_nerf_amd.config import lts_cfg
    from esr_nerf_amd.synthetic import slab_scene
    from oracle import ref_import
    ns = ref_import.load()
    cfg = lts_cfg("cpu", num_2ndrays=8, num_ltspts=12)
    sc = slab_scene("g16", s_val=60.0, oblique=True)
    torch.manual_seed(0)
    np.random.seed(0)
    model = ns.ESRNeRF(cfg, sc.near, sc.far, sc.xyz_min, sc.xyz_max, sc.mask_xyz_min, sc.mask_xyz_max,
                       sc.mask_alpha_init, sc.mask_density, sc.s_val, sc.num_voxels)
    with np.load(os.path.join(ROOT, "tests", "golden", "lts_g16_params.npz")) as z:
        model.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files})
    model.s_val = 60.0
    model.eval()
    pool = seeded_pool(model.xyz_min.numpy(), model.xyz_max.numpy())
    em = reference_attributes(model, torch.from_numpy(pool))["emission"]
    far = np.abs(em.max(1) - np.median(em.max(1))) > CLEAR * np.abs(em).max()
    pts = pool[far][:N_POINTS]
    assert len(pts) == N_POINTS, f"only {len(pts)} points of the pool lie outside the band"
    out = reference_attributes(model, torch.from_numpy(pts))
    k_val, gap = pick_k_val(out["emission"])
    scale = float(np.abs(out["emission"]).max())
    assert gap >= 4e-4 * scale, f"the widest gap {gap:.3e} is under 4e-4 x {scale:.3e}"
    out["k_val"] = k_val
    out["emissive"] = out["emission"].max(1) > k_val
    out = {k: np.ascontiguousarray(v) for k, v in out.items()}
    return out, gap, scale


def reference_attributes(model, pts):
    """the reference's own lines at explicit points"""
    with torch.no_grad():
        sdf, _ = model.sample_sdf_grad(pts.clone())
        _, expgrad = model.sample_sdf_expgrad(pts.clone())
        normal = F.normalize(expgrad.detach(), dim=-1)
        all_feat, _, all_normal = model.sample_sdfeat_grad_normal(pts.clone(), displace=model.grad_feat)
        rays_xyz = (pts - model.xyz_min) / (model.xyz_max - model.xyz_min)
        xyz_emb = (rays_xyz.unsqueeze(-1) * model.posfreq).flatten(-2)
        xyz_emb = torch.cat([rays_xyz, xyz_emb.sin(), xyz_emb.cos()], dim=-1)
        brdf_feat = torch.cat([xyz_emb, sdf[:, None], all_feat, all_normal], dim=-1)
        basecolor, roughness, metallic = model.brdfnet(torch.cat([model.brdf(pts), brdf_feat], dim=-1))
        emission = model.emitnet(torch.cat([model.emit_color(pts), brdf_feat], dim=-1))
    return dict(points=pts.numpy(), normal=normal.numpy(), sdf=sdf.numpy(), basecolor=basecolor.numpy(),
                roughness=roughness.reshape(-1).numpy(), metallic=metallic.reshape(-1).numpy(), emission=emission.numpy())


def main():
    out, gap, scale = generate()
    path = os.path.join(OUT, "surface_points.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} B): k_val {float(out['k_val']):.6g}, gap {gap:.3e} = "
          f"{gap / scale:.2e} max|emission|, {int(out['emissive'].sum())} of {N_POINTS} emissive, "
          f"|normal| in [{np.linalg.norm(out['normal'], axis=1).min():.6f}, {np.linalg.norm(out['normal'], axis=1).max():.6f}]")


if __name__ == "__main__":
    main()
