"""The options of `train` that run after training (train.AFTER_TRAINING): every one of them refuses a sharded run, a supervised run
and -- where it says so -- a K above 16, in the same words, on the command line and in train().  Parametrised over the table itself:
an option added there is covered by being there.  No GPU."""
import inspect

import numpy as np
import pytest
import torch

import neural_admixture_amd as na
from neural_admixture_amd import cli
from neural_admixture_amd.train import AFTER_KEYWORDS, AFTER_TRAINING

OPTIONS = pytest.mark.parametrize("opt", AFTER_TRAINING, ids=[o.kw for o in AFTER_TRAINING])


def _on(opt):
    """The smallest value that switches the option on: True for a switch, else 2 (rounds, folds or replicates)."""
    return True if inspect.signature(na.train).parameters[opt.kw].default is False else 2


def test_the_table_names_keywords_of_train():
    from neural_admixture_amd.model import Q_P
    ps = inspect.signature(na.train).parameters
    assert len(set(AFTER_KEYWORDS)) == len(AFTER_KEYWORDS)
    assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in AFTER_KEYWORDS)
    assert all(o.kw == o.params[0] for o in AFTER_TRAINING)
    assert Q_P(8, 8).after_results == {}


@OPTIONS
def test_cli_refuses_sharded_supervised_and_wide_runs(opt, tmp_path, monkeypatch):
    flag = "--" + opt.kw
    # no GPU where the option is refused before the GPU check (the refusal then shows the order too), one where it comes after it
    monkeypatch.setattr(torch.cuda, "is_available", lambda: not opt.cli_before_gpu)
    monkeypatch.setattr(cli, "_read", lambda *a, **kw: pytest.fail("the genotypes were read before the refusal"))
    base = ["train", "--name", "run", "--save_dir", str(tmp_path), "--data_path", str(tmp_path / "x.bed")]
    on = [flag] if _on(opt) is True else [flag, "2"]
    assert bool(getattr(cli.parse_train_args(base[1:] + ["--k", "3"] + on), opt.kw))
    assert not getattr(cli.parse_train_args(base[1:] + ["--k", "3"]), opt.kw)
    with pytest.raises(SystemExit, match=f"{flag} is single-GPU"):
        cli.main(base + ["--k", "3"] + on + ["--num_gpus", "2"])
    with pytest.raises(SystemExit, match=f"{flag} ignores labels"):
        cli.main(base + ["--k", "3"] + on + ["--pops_path", str(tmp_path / "absent.pop")])
    if opt.k16 is not None:
        for ks in (["--k", "17"], ["--min_k", "15", "--max_k", "17"]):
            with pytest.raises(SystemExit, match=rf"{flag} needs every K <= 16.*K = 17 was asked for"):
                cli.main(base + ks + on)
    assert not list(tmp_path.iterdir())


@OPTIONS
def test_train_refuses_sharded_supervised_and_wide_runs(opt):
    G0, V0, cpu = torch.zeros((4, 100), dtype=torch.uint8), np.zeros((8, 100), np.float32), torch.device("cpu")
    kw = {opt.kw: _on(opt)}
    with pytest.raises(ValueError, match=f"{opt.kw} needs a single-GPU, unsupervised run"):
        na.train(1, 8, 1e-3, 3, 0, G0, cpu, 2, 16, True, V0, None, **kw)
    with pytest.raises(ValueError, match=f"{opt.kw} needs a single-GPU, unsupervised run"):
        na.train(1, 8, 1e-3, 3, 0, G0, cpu, 1, 16, True, V0, ["a", "b", "c", "a"], **kw)
    if opt.k16 is not None:
        with pytest.raises(ValueError, match=f"{opt.kw} needs every K <= 16"):
            na.train(1, 8, 1e-3, 17, 0, G0, cpu, 1, 16, True, V0, None, **kw)
        with pytest.raises(ValueError, match=f"{opt.kw} needs every K <= 16"):
            na.train(1, 8, 1e-3, None, 0, G0, cpu, 1, 16, True, V0, None, 15, 17, **kw)
    with pytest.raises(RuntimeError, match="GPU"):               # in order: what is left is the device check
        na.train(1, 8, 1e-3, 3, 0, G0, cpu, 1, 16, True, V0, None, **kw)
