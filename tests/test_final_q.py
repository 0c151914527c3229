"""engine.final_q: the encoder's Q of all rows in batches -- what training, Engine.polish, Engine.kinship and Engine.snp_hwe end with."""
import torch


class _Rows:
    """Stands in for an engine: head h's Q of a batch is the batch's row numbers in column 0 and h in column 1."""
    device = torch.device("cpu")

    def __init__(self, heads):
        self.heads, self.calls = heads, []

    def infer_q(self, idx, b):
        assert idx.dtype == torch.int32 and idx.numel() == b
        self.calls.append(idx.tolist())
        return [torch.stack([idx.to(torch.float32), torch.full((b,), float(h))], dim=1) for h in range(self.heads)]


def test_final_q_covers_the_rows_in_order_with_a_short_last_batch():
    from neural_admixture_amd.engine import final_q, row_ranges
    assert row_ranges(70, 32) == [(0, 32), (32, 32), (64, 6)] and row_ranges(64, 32) == [(0, 32), (32, 32)] and row_ranges(5, 32) == [(0, 5)]
    eng = _Rows(2)
    Qs = final_q(eng, 70, 32)
    assert eng.calls == [list(range(0, 32)), list(range(32, 64)), list(range(64, 70))]
    assert len(Qs) == 2
    for h, Q in enumerate(Qs):
        assert Q.shape == (70, 2) and Q.dtype == torch.float32
        assert Q[:, 0].tolist() == [float(r) for r in range(70)] and (Q[:, 1] == float(h)).all()
