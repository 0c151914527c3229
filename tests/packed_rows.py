"""What the GPU tests of the analysis functions share (test_project_q, test_project_p, test_kinship, test_hwe, test_ld): the device,
packed rows made on the host and the row lists of test_hwe's and test_p_se's cases.  A plain module, imported the way the
``*_oracle`` modules are."""
import numpy as np
import torch


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def packed(Gm, dirty=False):
    """Packed rows [N, ld] on the host, ld = ceil(M/4) rounded up to 16 (the last chunk then reaches past the row's end); ``dirty``:
    every bit that holds no SNP set -- the unused fields of the last byte and the bytes behind it."""
    from neural_admixture_amd._lib import lib, check, ptr
    N, M = Gm.shape
    ld = ((M + 3) // 4 + 15) // 16 * 16
    out = torch.empty((N, ld), dtype=torch.uint8)
    check(lib.nadm_pack2bit_host(ptr(torch.from_numpy(np.ascontiguousarray(Gm))), ptr(out), N, M, ld), "pack2bit_host")
    if dirty:
        a = out.numpy()
        a[:, (M + 3) // 4:] = 0xFF
        if M % 4:
            a[:, M // 4] |= (0xFF << (2 * (M % 4))) & 0xFF
    return out


def case_rows(b, kind="list", resident=200):
    """The rows of a case: "none" = 0..b; "list" = a permutation of the resident rows with the one-hot row 2, the all-missing row 4
    and the 7-call row 5 in it, cut to b, the last entry a duplicate of the first (b = 1: row 7); b > ``resident``: drawn with
    repeats, the planted rows among them."""
    if kind == "none":
        return np.arange(b, dtype=np.int32)
    if b == 1:
        return np.asarray([7], dtype=np.int32)
    if b > resident:
        idx = np.random.default_rng(b).integers(0, resident, size=b).astype(np.int32)
        idx[[3, b // 2, b - 2]] = [2, 4, 5]
        return idx
    perm = np.random.default_rng(100 * b).permutation(resident)
    perm = np.concatenate([[2, 4, 5], perm[(perm != 2) & (perm != 4) & (perm != 5)]])[:b - 1]
    perm = perm[np.random.default_rng(100 * b + 1).permutation(b - 1)]
    return np.concatenate([perm, perm[:1]]).astype(np.int32)
