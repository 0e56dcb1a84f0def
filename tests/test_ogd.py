"""OGD on the host: constructor validation, the refusals of FusedAdamW, the state_dict schema, argument validation of the entry
points (which happens before any device work, so it runs without a GPU) and the float64 yardstick tests/test_ogd_gpu.py holds the
device to.

`gram_schmidt64` is classical Gram-Schmidt applied twice in float64 with the rule of cl.OGD.add_direction: a candidate is kept,
normalised, when the norm of its residual exceeds tol times its own norm (both over the scope), otherwise dropped.  The last
test checks the yardstick itself: its rows are orthonormal to 1e-13 and a dependent candidate is dropped."""
import pytest
import torch

from test_optimizer_clip_gpu import Toy, make_grad

STATE_KEYS = {"entries", "scope", "max_directions", "tol", "basis", "dependent", "nonfinite"}
STAT_KEYS = {"directions", "removed_fraction", "dependent", "nonfinite"}


def scope_mask(entries, numel, scope_names):
    """1.0 on the elements of the tensors in scope, 0.0 elsewhere (other tensors, the alignment gaps), float64."""
    m = torch.zeros(numel, dtype=torch.float64)
    for name, off, k, _ in entries:
        if name in scope_names:
            m[off:off + k] = 1.0
    return m


def residual64(rows, x):
    """x minus its components along the rows, twice (float64)."""
    for _ in range(2):
        if len(rows):
            R = torch.stack(rows)
            x = x - (R @ x) @ R
    return x


def gram_schmidt64(candidates, mask, tol=1e-3):
    """-> (rows, kept flags, residual ratios |r| / |g|), all float64."""
    rows, kept, ratios = [], [], []
    for g in candidates:
        g = g.double() * mask
        r = residual64(rows, g)
        ratio = float(r.norm() / g.norm())
        ratios.append(ratio)
        kept.append(ratio > tol)
        if kept[-1]:
            rows.append(r / r.norm())
    return rows, kept, ratios


def host_flat():
    from indic_cl_asr_amd import cl
    return cl.FlatParams(Toy(big=False))


def test_constructor_validation_and_scope():
    from indic_cl_asr_amd import cl
    flat = host_flat()
    for bad in (0, -1, cl.OGD_MAX_DIRECTIONS + 1):
        with pytest.raises(ValueError, match="max_directions"):
            cl.OGD(flat, bad)
    for bad in (0.0, -1e-3, 1.0, float("nan")):
        with pytest.raises(ValueError, match="tol"):
            cl.OGD(flat, 2, tol=bad)
    with pytest.raises(ValueError, match="matches no trainable tensor"):
        cl.OGD(flat, 2, scope="^nothing$")
    with pytest.raises(ValueError, match="not a trainable tensor"):
        cl.OGD(flat, 2, scope=["v1", "nope"])
    assert cl.OGD_MAX_DIRECTIONS >= 4096
    everything = cl.OGD(flat, 3)
    assert everything.scope_names == flat.names and everything.seg_scope.tolist() == [1] * len(flat.names)
    assert everything.basis.shape == (3, (flat.numel + 3) // 4 * 4) and everything.basis.dtype == torch.float32
    assert not everything.basis.any() and everything.directions == 0 and not everything.has_reference
    by_re = cl.OGD(flat, 1, scope=r"^v[0-3]$")
    assert by_re.scope_names == ["v0", "v1", "v2", "v3"]
    by_list = cl.OGD(flat, 1, scope=["mat", "v1"])
    assert by_list.scope_names == ["v1", "mat"]                    # layout order
    assert by_list.seg_scope.tolist() == [int(n in ("v1", "mat")) for n in flat.names]
    st = everything.stats()
    assert set(st) == STAT_KEYS and st["directions"] == 0 and st["removed_fraction"] != st["removed_fraction"]
    everything.clear()
    assert everything.directions == 0


def test_fused_adamw_refusals():
    from indic_cl_asr_amd import cl
    flat, other = host_flat(), host_flat()
    ogd = cl.OGD(flat, 2)
    with pytest.raises(ValueError, match="path_integral"):
        cl.FusedAdamW(flat, projection=ogd, path_integral=cl.SynapticIntelligence(flat))
    with pytest.raises(ValueError, match="masks"):
        cl.FusedAdamW(flat, projection=ogd, masks=cl.Piggyback(flat, masked=["mat"], frozen=[]))
    with pytest.raises(ValueError, match="another FlatParams"):
        cl.FusedAdamW(other, projection=ogd)
    opt = cl.FusedAdamW(flat, projection=ogd)
    assert opt.projection is ogd


def test_host_flat_params_raise_a_clear_error():
    from indic_cl_asr_amd import cl
    flat = host_flat()
    ogd = cl.OGD(flat, 2)
    flat.grad.fill_(1.0)
    with pytest.raises(RuntimeError, match="not on the device"):
        ogd.add_direction()
    assert ogd.directions == 0 and bool(flat.grad.all())            # nothing was consumed


def test_state_dict_schema_and_refusals(tmp_path):
    from indic_cl_asr_amd import checkpoint, cl
    flat = host_flat()
    ogd = cl.OGD(flat, 4, scope=["v1", "v9", "mat"], tol=1e-2)
    rows = torch.randn(2, flat.numel, generator=torch.Generator().manual_seed(5))
    ogd.basis[:2, :flat.numel].copy_(rows)
    ogd._rows, ogd.dependent, ogd.nonfinite = 2, 3, 1
    sd = ogd.state_dict()
    assert set(sd) == STATE_KEYS
    assert sd["entries"] == list(flat.entries) and sd["scope"] == ["v1", "v9", "mat"] and sd["max_directions"] == 4
    assert sd["basis"].shape == (2, flat.numel) and sd["basis"].device.type == "cpu" and torch.equal(sd["basis"], rows)
    assert (sd["dependent"], sd["nonfinite"], sd["tol"]) == (3, 1, 1e-2)
    path = str(tmp_path / "ogd.pt")
    checkpoint.save_projection(ogd, path)
    fresh = cl.OGD(host_flat(), 4, scope=["v1", "v9", "mat"])
    assert checkpoint.load_projection(fresh, path) is fresh
    assert fresh.directions == 2 and fresh.has_reference and torch.equal(fresh.basis[:2, :flat.numel], rows)
    assert not fresh.basis[2:].any() and (fresh.dependent, fresh.nonfinite) == (3, 1)
    with pytest.raises(ValueError, match="different scope"):
        cl.OGD(host_flat(), 4, scope=["v1", "mat"]).load_state_dict(sd)
    with pytest.raises(ValueError, match="max_directions"):
        cl.OGD(host_flat(), 1, scope=["v1", "v9", "mat"]).load_state_dict(sd)
    with pytest.raises(ValueError, match="different set of trainable tensors"):
        cl.OGD(cl.FlatParams(torch.nn.Linear(3, 2)), 4).load_state_dict(sd)
    assert fresh.stats()["directions"] == 2
    fresh.clear()
    assert fresh.directions == 0 and not fresh.has_reference


def test_entry_points_validate_before_any_device_work():
    import ctypes
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    assert L.ia_ogd_workspace_bytes(7, 3) == 7 * 4 * 4 and L.ia_ogd_workspace_bytes(7, 4096) == 7 * 4097 * 4
    assert L.ia_ogd_workspace_bytes(7, 0) == 0 and L.ia_ogd_workspace_bytes(7, 4097) == 0 and L.ia_ogd_workspace_bytes(0, 3) == 0
    buf = (ctypes.c_double * 64)()                                  # host memory: a valid, 16-byte aligned, non-NULL address
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def dots(x=p, basis=p, stride=8, numel=8, nrows=1, table=p, nchunks=1, nseg=1, scope=p, live=None, d64=p, d32=p, ws=p,
             ws_bytes=64):
        return L.ia_ogd_dots(x, basis, stride, numel, nrows, table, nchunks, nseg, scope, live, 1, d64, d32, ws, ws_bytes, None)

    def project(x=p, basis=p, stride=8, numel=8, nrows=1, coef=p, table=p, nchunks=1, nseg=1, scope=p, live=None, dst=p):
        return L.ia_ogd_project(x, basis, stride, numel, nrows, coef, 1.0, table, nchunks, nseg, scope, live, dst, None)

    for fn, required in ((dots, ("x", "basis", "table", "scope", "d64", "d32", "ws")),
                         (project, ("x", "basis", "coef", "table", "scope", "dst"))):
        for name in required:
            assert fn(**{name: None}) == -1, (fn.__name__, name)
        for nrows in (0, -1, 4097):
            assert fn(nrows=nrows) == -1
        for kw in (dict(stride=6), dict(stride=4), dict(stride=0), dict(stride=-8), dict(numel=0), dict(nchunks=0), dict(nseg=0)):
            assert fn(**kw) == -1, (fn.__name__, kw)                 # not a multiple of 4, below numel, empty
        for name in ("x", "basis"):
            assert fn(**{name: odd}) == -1, (fn.__name__, name)      # 16-byte alignment
    assert dots(d64=odd) == -1 and project(dst=odd) == -1
    assert dots(ws_bytes=7) == -2                                   # IA_WORKSPACE_TOO_SMALL, still before any launch


def test_float64_reference_yields_orthonormal_rows():
    flat = host_flat()
    entries, numel = list(flat.entries), flat.numel
    scope = [n for n in flat.names if n not in ("v3", "v8")]
    mask = scope_mask(entries, numel, scope)
    cands = [make_grad(entries, numel, 500 + k) for k in range(33)]
    cands.insert(20, 2.0 * cands[3].double() - 0.5 * cands[7].double())     # dependent on what is stored by then
    rows, kept, ratios = gram_schmidt64(cands, mask)
    assert kept == [True] * 20 + [False] + [True] * 13 and len(rows) == 33
    assert ratios[20] < 1e-12 and min(r for i, r in enumerate(ratios) if i != 20) > 0.1
    R = torch.stack(rows)
    assert float((R @ R.T - torch.eye(33, dtype=torch.float64)).abs().max()) <= 1e-13
    assert not bool((R * (1.0 - mask)).any())                       # zero outside the scope
