"""What the GPU tests of the analysis functions share (test_project_q, test_project_p, test_kinship, test_hwe, test_ld): the device and
packed rows made on the host.  A plain module, imported the way the ``*_oracle`` modules are."""
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
