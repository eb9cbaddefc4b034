"""CPU: the steps the harness entry points share (`harness.steps`) - the resolver contract with the plain model as one of the
resolvers, the keyword prologue, the score collector and the stats builder - around a stand-in module."""
import numpy as np
import pytest
import torch


class _Bilinear4(torch.nn.Module):
    """Stand-in with the drop-in call contract (B,7,C,H,W) -> (B,C,4H,4W): 4x bilinear of the centre frame plus the window mean."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.calls = []

    def forward(self, x):
        self.calls.append(tuple(x.shape))
        c = x[:, x.shape[1] // 2] * 0.5 + x.mean(1) * 0.5
        return torch.nn.functional.interpolate(c, scale_factor=4, mode="bilinear", align_corners=False) * self.w


def test_the_plain_model_is_a_resolver_on_the_padded_resident_frames():
    from fcvsr_amd.harness.steps import PlainResolver, Resolver, pad_to_multiple
    from fcvsr_amd.harness.windows import window_indices
    model = _Bilinear4()
    lr = torch.from_numpy(np.random.RandomState(0).rand(5, 1, 10, 12).astype(np.float32))
    res = PlainResolver(model)
    assert isinstance(res, Resolver) and res.multiple == 4
    x = pad_to_multiple(lr, res.multiple)
    assert tuple(x.shape) == (5, 1, 12, 12) and not x[:, :, 10:].any()
    idx = [window_indices(i, 7, 5, "replicate") for i in (0, 2, 4)]          # edge replication: rows repeat frames
    assert idx[0][:4] == [0, 0, 0, 0] and idx[2][-4:] == [4, 4, 4, 4]
    with torch.no_grad():
        got = res.sequence(x, idx)
        assert model.calls == [(3, 7, 1, 12, 12)]                            # one pass, nothing padded per batch
        want = model(torch.stack([x[j] for j in idx], 0))
        assert tuple(got.shape) == (3, 1, 48, 48) and torch.equal(got[..., :40, :48], want[..., :40, :48])
        assert torch.equal(res.frames(x, idx, "truncate", 10, 12), want[..., :40, :48])     # the group step: cropped by view
        assert torch.equal(res(torch.stack([x[j] for j in idx], 0)), want)                   # the window form


def test_resolver_for_always_returns_a_resolver():
    from fcvsr_amd.harness.ensemble import SelfEnsemble, for_mode
    from fcvsr_amd.harness.steps import PlainResolver, Resolver
    from fcvsr_amd.harness.tiles import TiledSuperResolver, resolver_for
    model = _Bilinear4()
    plain = resolver_for(model, None, None)
    assert isinstance(plain, PlainResolver) and plain.multiple == 4 and plain.model is model
    assert for_mode(model, None) is None                                      # the keyword's own helper keeps its answer
    for mode in ("spatial", "spatial+temporal"):
        ens = resolver_for(model, mode, None)
        assert isinstance(ens, SelfEnsemble) and isinstance(ens, Resolver) and ens.multiple == 1
        assert ens.temporal == (mode == "spatial+temporal")
    tiled = resolver_for(model, "spatial", 12, 4, batch=3)
    assert isinstance(tiled, TiledSuperResolver) and isinstance(tiled, Resolver) and tiled.multiple == 1
    # its model passes are limited to the harness's batch (the passes themselves run on the HIP device only: test_tiles_gpu.py)
    assert tiled.batch == 3 and tiled.tile == (12, 12) and tiled.tile_overlap == (4, 4) and tiled.ensemble == "spatial"
    assert TiledSuperResolver(model, 12, 4).batch == 8                        # the default of direct users
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tiled.sequence(torch.zeros(3, 1, 10, 12), [[0, 1, 2]])


def test_the_prologue_validates_every_keyword_and_returns_the_resolver():
    from fcvsr_amd.harness.steps import PlainResolver, check_keywords
    good = dict(ensemble=None, tile=None, tile_overlap=16, batch=2, quantise="truncate", cuts=None, frame_dtype=torch.float32)
    model = object()                                                          # never looked at
    assert isinstance(check_keywords(model, **good), PlainResolver)
    for change, word in ((dict(ensemble="x8"), "ensemble"), (dict(tile=30), "tile"), (dict(tile=16, tile_overlap=9), "tile_overlap"),
                         (dict(batch=0), "batch"), (dict(quantise="bogus"), "quantise"), (dict(cuts="detect"), "auto"),
                         (dict(cuts="auto"), "explicit cuts"), (dict(channels=(1,), who="f"), "one-channel"),
                         (dict(channels=(1, 3), who="f"), r"one-channel \(Y\) or three-channel \(RGB\)")):
        with pytest.raises(ValueError, match=word):
            check_keywords(model, **{**good, **change})
    assert check_keywords(model, **{**good, "cuts": "auto", "frame_dtype": torch.uint8}).multiple == 4


def test_quantise_is_validated_on_the_float_path_of_super_resolve_sequence():
    from fcvsr_amd.harness.infer import super_resolve_sequence
    lr = torch.rand(3, 1, 8, 8)
    with pytest.raises(ValueError, match="quantise"):
        super_resolve_sequence(_Bilinear4(), lr, quantise="bogus")
    assert super_resolve_sequence(_Bilinear4(), lr, quantise="round").shape == (3, 1, 32, 32)


def test_the_score_collector_without_scores_and_the_stats_builder():
    from fcvsr_amd.harness.steps import ScoreCollector, run_stats
    col = ScoreCollector()
    feats = col.features(torch.zeros(2, 1, 96, 192, dtype=torch.uint8))      # nothing was asked for: nothing runs
    assert feats == (None, None)
    col.add(feats)
    assert col.stats() == {}
    stats = run_stats(9, 0.5, 100, 1600, (80, 72), col.stats(), None)
    assert stats == {"frames": 9, "seconds": 0.5, "fps": 18.0, "bytes_read": 100, "bytes_written": 1600, "out_size": (80, 72)}
    assert "cuts" not in stats and list(stats)[:3] == ["frames", "seconds", "fps"]
    with_cuts = run_stats(9, 0.0, 100, 1600, (80, 72), {"niqe_mean": 4.0}, [])
    assert with_cuts["cuts"] == [] and with_cuts["niqe_mean"] == 4.0 and with_cuts["fps"] == float("inf")


def test_the_score_check_takes_the_bit_depth_and_the_scored_size(golden_dir):
    import os
    from fcvsr_amd.harness.niqe import NiqeModel
    from fcvsr_amd.harness.steps import check_scores
    from fcvsr_amd.harness.yuv import _check_niqe
    niqe = NiqeModel.load(os.path.join(golden_dir, "niqe_pris_params.npz"))
    assert check_scores(None, None, 10, 2, 2) is None                         # no keyword, nothing to refuse
    assert check_scores(niqe, None, 8, 96, 192) is None
    _check_niqe(niqe, 8, 48, 24)                                             # the file paths' form: LR width x height
    with pytest.raises(ValueError, match="8-bit"):
        check_scores(niqe, None, 10, 96, 192)
    with pytest.raises(ValueError):
        check_scores(niqe, None, 8, 96, 191)                                 # fewer than two blocks
    with pytest.raises(ValueError, match="BrisqueModel"):
        check_scores(None, object(), 8, 96, 192)
