"""bench.py --dump-outputs without a GPU: what it keeps of a step's results and how it stays inside its size budget."""
import numpy as np
import torch

import bench


def _gathered(cap):
    sym = torch.arange(3 * cap, dtype=torch.uint8) + 65
    return [(sym, torch.tensor([2, 0, 5], dtype=torch.int32), torch.tensor([1.5, -2.0, 3.25], dtype=torch.float64),
             torch.tensor([0, 1, 0], dtype=torch.uint8))]


def test_symbols_past_the_decoded_length_are_zero():
    o = bench.viterbi_outputs(_gathered(5), 5)
    assert o["symbols"].tolist() == [[65, 66, 0, 0, 0], [0] * 5, [75, 76, 77, 78, 79]]
    assert o["length"].tolist() == [2, 0, 5] and o["loglike"].tolist() == [1.5, -2.0, 3.25] and o["status"].tolist() == [0, 1, 0]
    assert o["read_index"].tolist() == [0, 1, 2]
    assert o["loglike"].dtype == o["read_index"].dtype == np.float64 and all(o[n].dtype == np.float32 for n in ("symbols", "length", "status"))


def test_a_large_output_is_a_fixed_sample(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * (4 * 5 + 24))
    a, b = bench.viterbi_outputs(_gathered(5), 5), bench.viterbi_outputs(_gathered(5), 5)
    assert len(a["read_index"]) == 2 and a["read_index"].tolist() == b["read_index"].tolist()
    for i, r in enumerate(a["read_index"].astype(int)):
        assert a["loglike"][i] == [1.5, -2.0, 3.25][r]
    bench.write_outputs(str(tmp_path), a)
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 * 10 ** 6
    assert np.load(str(tmp_path / "loglike.npy")).tolist() == a["loglike"].tolist()
