"""Same work under two builds of the library (NADM_LIB): run once per build, in a process of its own, and compare the printed lines.
  (no argument)   a checksum of every parameter after 6 training steps on a few shapes
  headline        the same at the headline shape (800 rows of 500k SNPs, K = 8), a K <= 4 and a K = 16 shape instead
  analyses        a sha256 of every output buffer of nadm_kinship, nadm_ibd, nadm_sample_info, nadm_resid_project and nadm_project_q
                  (with the log-likelihood) on inputs from a seeded numpy generator: ragged tiles, a ragged last chunk, several ranges,
                  ranges of several chunks, waves without a row, gather lists and none, a pimin that masks"""
import os, sys, hashlib, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import neural_admixture_amd as na
dev = torch.device("cuda:0")


def sha(*ts):
    return " ".join(hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16] for t in ts)


def analyses():
    from neural_admixture_amd import project, qse, relate, residpca
    from neural_admixture_amd._lib import lib
    from neural_admixture_amd._packed import pad_P, pad_Q
    from neural_admixture_amd.layout import ModelLayout
    rng = np.random.default_rng(20)

    def model(rows, M, K):                                    # random calls (a quarter missing, pad bits set), P and Q of the head
        xp = torch.from_numpy(rng.integers(0, 256, (rows, ModelLayout.row_stride(M)), dtype=np.uint8)).to(dev)
        P = rng.uniform(0.02, 0.98, (M, K)).astype(np.float32)
        Q = rng.dirichlet(0.3 * np.ones(K), size=rows).astype(np.float32)
        return xp, pad_P(P, dev), Q, int(lib.nadm_pad_k(K))

    def gather(rows, b):
        return torch.from_numpy(rng.permutation(rows)[:b].astype(np.int32)).to(dev)

    for ba, bb, M in ((70, 130, 1027), (15, 17, 300001)):
        for K in (3, 8, 16, 33):
            rows = ba + bb + 9
            xp, Pp, Q, kp = model(rows, M, K)
            for lists, pimin in ((True, 0.05), (False, 0.0)):
                # without lists both sides are the matrix's first rows
                ia, ib = (gather(rows, ba), gather(rows, bb)) if lists else (None, None)
                QA = pad_Q(Q[ia.cpu().numpy()] if lists else Q[:ba], ba, K, kp, dev)
                QB = pad_Q(Q[ib.cpu().numpy()] if lists else Q[:bb], bb, K, kp, dev)
                tag = f"({ba}, {bb}, {M}) K={K} lists={int(lists)} pimin={pimin}"
                print("kinship", tag, sha(*relate.kinship_block(xp, M, Pp, K, ia, QA, ib, QB, pimin)))
                if K <= 16:
                    fA, fB = (torch.from_numpy(rng.uniform(-0.1, 0.1, n).astype(np.float32)).to(dev) for n in (ba, bb))
                    print("ibd    ", tag, sha(*relate.ibd_block(xp, M, Pp, K, ia, QA, fA, ib, QB, fB, pimin)))
    for b, M in ((300, 1027), (70, 300001)):
        for K in (3, 16):
            rows = b + 9
            xp, Pp, Q, kp = model(rows, M, K)
            for lists in (True, False):
                idx = gather(rows, b) if lists else None
                xb = xp if lists else xp[:b].contiguous()
                Qb = Q[idx.cpu().numpy()] if lists else Q[:b]
                tag = f"({b}, {M}) K={K} lists={int(lists)}"
                print("sample_info  ", tag, sha(*qse.q_info(xb, M, Pp[:, :K], Qb, idx)))
                for CP in (16, 32):
                    W = torch.zeros((M, CP), dtype=torch.float32, device=dev)
                    W[:, :CP - 3] = torch.from_numpy(rng.standard_normal((M, CP - 3)).astype(np.float32)).to(dev)
                    Y = residpca._project(xb, M, K, Pp, pad_Q(Qb, b, K, kp, dev), idx, b, W, CP - 3, 0.05 if lists else 0.0, residpca.EPS)
                    print("resid_project", tag, f"CP={CP}", sha(*Y))
    b, M = 70, 1027
    for K in (3, 33):
        xp, Pp, Q, kp = model(b + 9, M, K)
        for lists in (True, False):
            idx = gather(b + 9, b) if lists else None
            qin = pad_Q(Q[:b], b, K, kp, dev)
            qout, ll, n = torch.empty_like(qin), torch.empty(b, dtype=torch.float64, device=dev), torch.empty(b, dtype=torch.int32, device=dev)
            scratch = torch.empty(max(int(lib.nadm_project_scratch_floats(b, M, kp)), 4), dtype=torch.float32, device=dev)
            project.em_step(xp, M, idx, b, Pp, K, qin, qout, scratch, loglik=ll, nobs=n)
            print("project_q", f"({b}, {M}) K={K} lists={int(lists)}", sha(qout, ll, n))
    torch.cuda.synchronize()


if sys.argv[1:] == ["analyses"]:
    analyses()
    sys.exit(0)

from oracle import nadm_oracle as O
SHAPES = ((900, 70_001, [8], 800), (300, 5003, [3], 100), (500, 20_000, [2, 5, 8], 333), (4500, 20_000, [7], 4301), (4400, 9_000, [2, 3, 9], 4099))
if sys.argv[1:] == ["headline"]:
    SHAPES = ((900, 500_000, [8], 800), (300, 5003, [3], 100), (400, 60_000, [16], 333))
for (N, M, ks, b) in SHAPES:
    G = O.synth_genotypes(N, M, max(ks), seed=5, missing=0.02)
    rng = np.random.default_rng(1)
    V0 = (rng.standard_normal((M, 8)) / np.sqrt(M)).astype(np.float32)
    P0 = rng.uniform(0.02, 0.98, (sum(ks), M)).astype(np.float32)
    e = na.Engine(M, 8, 256, ks, dev, b)
    e.load_params(V0, P0, na.model.init_encoder_weights(3, 8, 256, ks))
    e.pack_from_host(torch.from_numpy(G))
    idx = torch.from_numpy(rng.permutation(N).astype(np.int32)).to(dev)
    for s in range(6):
        bb = b if s != 3 else b - 37
        e.train_step(idx[:bb], bb, 2e-3, True)
    e.sync(); torch.cuda.synchronize()
    print(N, M, ks, b, hashlib.sha256(e.pflat.cpu().numpy().tobytes()).hexdigest()[:16], e.read_loss()[1])
