"""The tiled, cleaned resident copy of the genotype matrix (nadm_tile_packed, Engine(resident=...)).

The copy is made once when the matrix is handed over; the step's matrix-core passes then gather the batch out of it instead of out of the
row-major matrix.  The same codes enter the same arithmetic in the same order, so everything here that compares the two sources asks for
EXACT equality: parameters, moments, loss and Q.  The host side (descriptor checks, size query, refusals and their order) is
csrc/host_selfcheck_tiles.cpp, built and run below without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

gpu = pytest.mark.gpu
CW, HD = 8, 64


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _genotypes(N, M, seed, missing=0.03):
    """Codes 0 / 1 / 2 with `missing` of the calls 3; code 3 planted in the first and last rows and SNPs."""
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 3, size=(N, M), dtype=np.uint8)
    G[rng.random((N, M)) < missing] = 3
    G[0, :5] = 3; G[0, -5:] = 3; G[-1, :5] = 3; G[-1, -5:] = 3; G[:, 0][::7] = 3; G[:, -1][::5] = 3
    return G


def _params(M, ks, seed):
    rng = np.random.default_rng(seed)
    V0 = (rng.standard_normal((M, CW)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.05, 0.95, size=(sum(ks), M)).astype(np.float32)
    parts = [np.ones(CW), rng.standard_normal(HD * CW) / np.sqrt(CW), np.zeros(HD)]
    for k in ks:
        parts += [rng.standard_normal(k * HD) / np.sqrt(HD), np.zeros(k)]
    return V0, P0, np.concatenate(parts).astype(np.float32)


def _engine(G, ks, bmax, params, cls=None, **kw):
    import neural_admixture_amd as na
    M = G.shape[1]
    e = (cls or na.Engine)(M, CW, HD, ks, _dev(), bmax, **kw)
    e.load_params(*params)
    e.pack_from_host(torch.from_numpy(G))
    return e


def _batch(N, b, seed):
    """b rows with rows 0 and N - 1 and one row twice."""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(N)[:b].astype(np.int32)
    idx[0], idx[1], idx[2] = 0, N - 1, idx[3]
    return idx


def _state(e, idx, b, steps=3):
    dev = e.device
    for s in range(steps):
        e.train_step(torch.from_numpy(np.roll(idx, s)).to(dev), b, 2e-3, True)
    e.sync()
    torch.cuda.synchronize()
    return {"params": e.pflat.clone(), "m": e.mflat.clone(), "v": e.vflat.clone(), "Q": e.Q.clone(), "loss": e.read_loss()}


def _same(a, b, what):
    assert a["loss"] == b["loss"], (what, a["loss"], b["loss"])
    for k in ("params", "m", "v", "Q"):
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))
    assert bool(torch.isfinite(a["params"]).all())


def _rows_vs_tiled(G, ks, b, idx, **kw):
    """Three steps from the row-major matrix and from the tiled copy (pass 3 from pass 2's batch copy, then from the tiled copy too)."""
    params = _params(G.shape[1], ks, 5)
    ref_e = _engine(G, ks, b, params, resident="rows", **kw)
    assert ref_e._xt is None
    ref = _state(ref_e, idx, b)
    del ref_e
    for p3 in (False, True):
        e = _engine(G, ks, b, params, resident="tiled", resident_pass3=p3, **kw)
        assert e._xt is not None and e._xt.numel() == 128 * G.shape[0] * ((G.shape[1] + 511) // 512)
        assert (e._xg is None) == p3                              # pass 3 from the copy: no batch copy is allocated
        _same(_state(e, idx, b), ref, f"resident_pass3={p3}")
        del e


# ------------------------------------------------------------------------------------------------ 1. the copy itself
@gpu
@pytest.mark.parametrize("N,M,ld", [(37, 1000, 272), (300, 5003, None)])
def test_tile_packed_against_a_numpy_relayout(N, M, ld):
    from neural_admixture_amd._lib import lib, check, ptr
    dev = _dev()
    mp = (M + 3) // 4
    ld = ld or ((mp + 15) // 16) * 16
    rng = np.random.default_rng(N)
    xp = rng.integers(0, 256, size=(N, ld), dtype=np.uint8)         # every code, code 3 everywhere, pad bytes and pad bits set
    for r in (0, N - 1):                                            # code 3 in the first and last rows: first SNP, last SNP, the byte that straddles M
        xp[r, 0] |= 0x03
        xp[r, (M - 1) // 4] |= 0x03 << (2 * ((M - 1) % 4))
        xp[r, (M - 1) // 4] |= 0xC0
    codes = np.stack([(xp >> (2 * i)) & 3 for i in range(4)], axis=-1).reshape(N, ld * 4)
    codes[:, M:] = 0
    codes[codes == 3] = 0
    tiles = (M + 511) // 512
    wide = np.zeros((N, tiles * 512), dtype=np.uint8)
    wide[:, : min(ld * 4, tiles * 512)] = codes[:, : tiles * 512]
    packed = (wide.reshape(N, tiles * 128, 4) << (2 * np.arange(4, dtype=np.uint8))).sum(axis=-1).astype(np.uint8)
    want = packed.reshape(N, tiles, 128).transpose(1, 0, 2).copy()  # [tile][row][128 B]
    need = int(lib.nadm_tiled_bytes(N, M))
    assert need == tiles * N * 128
    xd = torch.from_numpy(xp).to(dev)
    xt = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    check(lib.nadm_tile_packed(ptr(xd), ld, N, M, ptr(xt), None), "tile_packed")
    torch.cuda.synchronize()
    got = xt.cpu().numpy()
    assert np.array_equal(got[:need].reshape(tiles, N, 128), want)
    assert (got[need:] == 0xA5).all()                               # nothing behind the copy is written
    assert (want.reshape(tiles, N, 128)[-1][:, (mp - (tiles - 1) * 128):] == 0).all()      # the pad bytes of the last tile


# ------------------------------------------------------------------------------------------------ 2. bit identity of the step
@gpu
@pytest.mark.parametrize("K", [3, 8, 16])
@pytest.mark.parametrize("b", [33, 70, 130])
def test_step_from_the_tiled_copy_is_bit_identical(K, b):
    N, M = 150, 5003
    _rows_vs_tiled(_genotypes(N, M, 1), [K], b, _batch(N, b, b))


@gpu
@pytest.mark.parametrize("M", [5003, 25000])
def test_sliced_pass2_from_the_tiled_copy_is_bit_identical(M):
    from neural_admixture_amd._lib import lib
    N, b = 820, 800
    assert int(lib.nadm_decode_slices(b, M, 8)) > 1
    _rows_vs_tiled(_genotypes(N, M, 2), [8], b, _batch(N, b, 3))


@gpu
def test_sliced_pass3_from_the_tiled_copy_is_bit_identical():
    from neural_admixture_amd._lib import lib
    N, b, M = 4100, 4000, 3000                                     # 6 chunks of 512 SNPs (< 192), 32 tiles of 128 samples
    assert int(lib.nadm_encode_slices(b, M, CW)) > 1
    _rows_vs_tiled(_genotypes(N, M, 3), [8], b, _batch(N, b, 4))


@gpu
def test_dp_buckets_from_the_tiled_copy_are_bit_identical():
    from neural_admixture_amd.comm import emulated_comm
    N, b, M = 150, 70, 9001
    comm = emulated_comm(2)
    try:
        import neural_admixture_amd as na
        assert na.Engine(M, CW, HD, [8], _dev(), b, mode="dp", comm=comm, n_buckets=3).lay.n_buckets == 3
        _rows_vs_tiled(_genotypes(N, M, 4), [8], b, _batch(N, b, 5), mode="dp", comm=comm, n_buckets=3)
    finally:
        comm.close()


@gpu
def test_snp_sharded_engine_tiles_its_own_slice():
    from neural_admixture_amd.comm import rccl_comm
    from neural_admixture_amd.snp_parallel import SnpShardedEngine
    N, b, M = 150, 70, 5003
    comm = rccl_comm(0, 1)
    try:
        _rows_vs_tiled(_genotypes(N, M, 5), [8], b, _batch(N, b, 6), cls=SnpShardedEngine, comm=comm)
    finally:
        comm.close()


@gpu
@pytest.mark.parametrize("K", [3, 8, 16])
def test_medium_step_from_the_tiled_copy_is_bit_identical(K):
    N, b, M = 150, 130, 5003
    _rows_vs_tiled(_genotypes(N, M, 6), [K], b, _batch(N, b, 7), precision="medium")


# ------------------------------------------------------------------------------------------------ 3. missing = 1.5 reads the raw matrix
@gpu
def test_pca_projection_reads_the_raw_matrix_beside_a_resident_copy():
    from neural_admixture_amd._lib import lib, check, ptr
    N, M, b = 150, 5003, 70
    G = _genotypes(N, M, 7, missing=0.1)
    params = _params(M, [8], 5)
    idx = _batch(N, b, 8)
    Vd = torch.from_numpy(params[0]).to(_dev()).contiguous()
    out = []
    for res in ("rows", "tiled"):
        e = _engine(G, [8], b, params, resident=res, resident_pass3=True)
        _state(e, idx, b, steps=1)                                  # the plan has read its source
        chunks = int(lib.nadm_encode_chunks(M))
        zpart = torch.zeros(chunks * b * CW, dtype=torch.float32, device=e.device)
        check(lib.nadm_pca_project(ptr(e.xp), e.ld, ptr(torch.from_numpy(idx).to(e.device)), b, M, ptr(Vd), CW, ptr(zpart), None), "pca_project")
        torch.cuda.synchronize()
        out.append(zpart.view(chunks, b, CW).double().sum(0).cpu().numpy())
    assert np.array_equal(out[0], out[1])
    x = G[idx].astype(np.float64) / 2.0                              # code 3 is 1.5: the copy, which holds no code 3, would give less
    want = x @ params[0].astype(np.float64)
    assert (G[idx] == 3).sum() > 1000
    # fp32 accumulation over M terms of magnitude <= 1.5 |V|: M * 2^-24 * sum |x v| bounds the rounding (the products are exact)
    bound = M * 2.0 ** -24 * (np.abs(x) @ np.abs(params[0].astype(np.float64))).max()
    assert np.abs(out[1] - want).max() <= bound
    assert np.abs((np.where(G[idx] == 3, 0, G[idx]) / 2.0) @ params[0].astype(np.float64) - want).max() > 100 * bound


# ------------------------------------------------------------------------------------------------ 4. a tile offset past 4 GiB
@gpu
def test_tile_offset_past_4_gib():
    import neural_admixture_amd as na
    from neural_admixture_amd._lib import lib, check, ptr
    dev = _dev()
    N, M, K, b = 70000, 250000, 8, 48
    params = _params(M, [K], 9)
    g = torch.Generator(device="cpu").manual_seed(0)
    Qt = torch.distributions.Dirichlet(torch.full((K,), 0.2)).sample((N,)).float().to(dev)
    Fq = (0.5 * torch.rand(K, M, generator=g)).clamp(0.005, 0.5).to(dev)
    idx = np.concatenate([[0, N - 1, N - 1], np.random.default_rng(1).permutation(N)[: b - 3]]).astype(np.int32)
    got = []
    xp = None
    for res in ("rows", "tiled"):
        e = na.Engine(M, CW, HD, [K], dev, b, resident=res, resident_pass3=True)
        if xp is None:
            xp = torch.empty((N, e.ld), dtype=torch.uint8, device=dev)
            check(lib.nadm_synth_packed(ptr(xp), N, 0, M, e.ld, ptr(Qt), ptr(Fq), K, 0.02, 1234, None), "synth_packed")
        e.load_params(*params)
        e.set_packed(xp)
        if res == "tiled":
            assert e._xt.numel() == 489 * N * 128 and (M // 512) * N * 128 > 1 << 32       # the tiles from 480 on start past 4 GiB
        got.append(_state(e, idx, b, steps=1))
        del e
    _same(got[1], got[0], "tile offset past 4 GiB")


# ------------------------------------------------------------------------------------------------ 5. the fallback
@gpu
def test_forced_and_simulated_fallback_train_like_the_default(monkeypatch):
    from neural_admixture_amd import engine as E
    N, M, b = 150, 5003, 70
    G, params, idx = _genotypes(N, M, 8), _params(M, [8], 5), _batch(N, b, 9)
    e = _engine(G, [8], b, params)                                   # "auto": the copy fits
    assert e._xt is not None
    default = _state(e, idx, b)
    del e
    e = _engine(G, [8], b, params, resident="rows")
    assert e._xt is None
    _same(_state(e, idx, b), default, "resident='rows'")
    del e
    monkeypatch.setattr(E, "_copy_fits", lambda device, need: False)
    e = _engine(G, [8], b, params)                                   # "auto": does not fit
    assert e._xt is None and e._xg is not None
    _same(_state(e, idx, b), default, "does not fit")
    del e
    e = _engine(G, [8], b, params, resident="tiled")                 # forced: the question is not asked
    assert e._xt is not None
    _same(_state(e, idx, b), default, "resident='tiled'")
    with pytest.raises(ValueError, match="resident"):
        _engine(G, [8], b, params, resident="tiles")


@gpu
def test_a_matrix_written_in_place_is_tiled_again():
    """The engine's matrix is a live operand of the step: after an in-place write into eng.xp the step reads the new rows, as it does from
    the row-major matrix."""
    N, M, b = 150, 5003, 70
    G1, G2, params, idx = _genotypes(N, M, 10), _genotypes(N, M, 11), _params(M, [8], 5), _batch(N, b, 12)
    ref = _engine(G1, [8], b, params, resident="rows")
    _state(ref, idx, b, steps=1)
    e = _engine(G1, [8], b, params, resident="tiled")
    _state(e, idx, b, steps=1)
    other = _engine(G2, [8], b, params, resident="rows").xp
    for eng in (ref, e):
        eng.xp.copy_(other)
    xt = e._xt
    want, got = _state(ref, idx, b, steps=2), _state(e, idx, b, steps=2)
    _same(got, want, "after an in-place write")
    assert e._xt is xt                                               # made again where it was: no second 12.5 GB


# ------------------------------------------------------------------------------------------------ 6. the host side, no GPU
def test_header_and_library_carry_the_tiled_copy():
    from neural_admixture_amd._lib import lib
    hdr = open(os.path.join(ROOT, "include", "nadm.h")).read()
    for name in ("nadm_tiled_bytes", "nadm_tile_packed", "nadm_plan_set_tiles"):
        assert name + "(" in hdr and hasattr(lib, name)
    assert lib.nadm_tiled_bytes(37, 1000) == 2 * 37 * 128 and lib.nadm_tiled_bytes(100000, 500000) == 977 * 100000 * 128
    assert lib.nadm_tiled_bytes(5, 512) == 5 * 128 and lib.nadm_tiled_bytes(5, 513) == 2 * 5 * 128
    assert lib.nadm_tiled_bytes(0, 100) == 0 and lib.nadm_tiled_bytes(3, 0) == 0
    assert lib.nadm_plan_set_tiles(None, None, 0, 0) != 0 and b"null pointer" in lib.nadm_last_error()
    buf = (C.c_uint8 * 64)()
    assert lib.nadm_tile_packed(None, 16, 1, 4, buf, None) != 0 and b"null pointer" in lib.nadm_last_error()


def test_host_selfcheck_of_the_tiled_source_builds_and_passes(tmp_path):
    """csrc/host_selfcheck_tiles.cpp as a plain program (no GPU): the descriptor's checks in the three passes, the size query at ragged M,
    the refusals of nadm_tile_packed and their order, against launchers that only record."""
    csrc = os.path.join(ROOT, "neural-admixture_amd", "csrc")
    exe = str(tmp_path / "host_selfcheck_tiles")
    units = ["host_selfcheck_tiles.cpp", "nadm_host_io.cpp", "nadm_layout.cpp", "nadm_passes_host.cpp", "nadm_hooks.cpp"]
    import shutil
    cxx = shutil.which("hipcc") or shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    cc = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-o", exe] + [os.path.join(csrc, u) for u in units] + ["-lpthread", "-ldl"],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("host_selfcheck_tiles ok"), (run.stdout, run.stderr)
