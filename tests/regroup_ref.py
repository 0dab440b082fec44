"""Restatement of PDRA's ray re-split (esr_nerf_amd/regroup.py over csrc/regroup.hip) in numpy: the decision
(app/fine/pdra.py:911), the statistics (:912-925, over non-NaN values) and the stable partition of
``RayGroupManager.filter`` (utils2/utils.py:234-267), with five named mutants, and the shared inputs of
tests/test_regroup_host.py and tests/test_gpu_regroup.py."""
import numpy as np

MUTANTS = ("ge", "min_channel", "nan_uncertain", "unstable", "front")
TILE = 1024                                      # ESR_PARTITION_BLOCK (the unit inside which the `unstable` mutant reorders)
STAT_KEYS = ("n_set", "n_clear", "n_nan", "min_all", "max_all", "min_set", "max_set", "min_clear", "max_clear")


def decide(emission, k_val, mutant=None):
    """flags [n] bool: max over the channels > k_val as binary32; a ray with a NaN channel is not set"""
    e = np.asarray(emission, np.float32).reshape(-1, 3)
    k = np.float32(k_val)
    nan = np.isnan(e).any(1)
    with np.errstate(invalid="ignore"):
        m = (np.fmin if mutant == "min_channel" else np.fmax).reduce(e, axis=1) if len(e) else np.zeros(0, np.float32)
        hit = m >= k if mutant == "ge" else m > k            # (fmax skips a NaN: the NaN rule is the line below)
    return hit if mutant == "nan_uncertain" else hit & ~nan


def order_key(v):
    """int32 keys of a total order on non-NaN binary32 values with -0.0 below +0.0"""
    b = np.asarray(v, np.float32).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7fffffff))


def _lo_hi(values):
    v = values[~np.isnan(values)]
    if not v.size:
        return np.float32(np.inf), np.float32(-np.inf)
    k = order_key(v)
    return v[np.argmin(k)], v[np.argmax(k)]


def stats(emission, flags):
    """The record of esr_regroup_stats_t as a dict (float entries are np.float32 scalars, compared by bits)"""
    e = np.asarray(emission, np.float32).reshape(-1, 3)
    f = np.asarray(flags, bool)
    (la, ha), (ls, hs), (lc, hc) = _lo_hi(e.reshape(-1)), _lo_hi(e[f].reshape(-1)), _lo_hi(e[~f].reshape(-1))
    return dict(n_set=int(f.sum()), n_clear=int((~f).sum()), n_nan=int(np.isnan(e).any(1).sum()), min_all=la, max_all=ha,
                min_set=ls, max_set=hs, min_clear=lc, max_clear=hc)


def same_stats(got, want):
    """bit equality of two records (got: python floats / ints or numpy scalars)"""
    bad = [k for k in STAT_KEYS
           if (int(got[k]) != int(want[k]) if k.startswith("n_")
               else np.float32(got[k]).view(np.uint32) != np.float32(want[k]).view(np.uint32))]
    return bad


def partition(uncert, cert, flags, mutant=None):
    """(new uncertain, new certain): set rows stay in order, clear rows go to the END of the certain vector in order"""
    u, c, f = np.asarray(uncert, np.int64), np.asarray(cert, np.int64), np.asarray(flags, bool)
    keep, moved = u[f], u[~f]
    if mutant == "unstable":                     # the set rows of each tile leave in reverse
        parts = [u[a:a + TILE][f[a:a + TILE]][::-1] for a in range(0, len(u), TILE)]
        keep = np.concatenate(parts) if parts else keep
    return keep, (np.concatenate([moved, c]) if mutant == "front" else np.concatenate([c, moved]))


def edge_rows(k_val):
    """Rays around the decision and the number formats: a channel equal to k_val, one ulp either side, NaN in each channel
    (with and without another channel above k_val), +-inf, -0.0 / +0.0"""
    k = np.float32(k_val)
    up, dn = np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-np.inf))
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    lo = np.float32(k - abs(k) - 1.0)
    return np.array([[k, lo, lo], [lo, k, dn], [up, lo, lo], [lo, dn, lo], [dn, dn, up], [k, k, k],
                     [nan, lo, lo], [lo, nan, up], [up, up, nan], [nan, nan, nan], [inf, lo, lo], [-inf, -inf, -inf],
                     [lo, -inf, inf], [-0.0, 0.0, -0.0], [0.0, -0.0, lo], [-0.0, -0.0, -0.0]], np.float32)


def emission_case(n, k_val, seed, edges=True):
    """[n, 3] float32 softplus-like values around k_val, the edge rows planted at seeded positions when they fit"""
    rng = np.random.default_rng(seed)
    e = (np.float32(k_val) + rng.standard_normal((n, 3)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    if edges and n:
        rows = edge_rows(k_val)
        m = min(n, len(rows))
        where = rng.choice(n, size=m, replace=False)
        e[where] = rows[rng.permutation(len(rows))[:m]]
    return e


def flag_patterns(n, seed):
    """name -> [n] bool: all set, all clear, alternating, runs of 1 .. 4097, random at 1 % and 99 %"""
    rng = np.random.default_rng(seed)
    runs = []
    while sum(runs) < n:
        runs.append(int(rng.integers(1, 4098)) if len(runs) % 3 else int(rng.integers(1, 5)))
    run = np.concatenate([np.full(r, i % 2 == 0) for i, r in enumerate(runs)])[:n] if n else np.zeros(0, bool)
    if n > 4097:
        run[:4097] = True                        # the longest run, whole
    return {"all_set": np.ones(n, bool), "all_clear": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0, "runs": run,
            "random_1": rng.random(n) < 0.01, "random_99": rng.random(n) < 0.99}
