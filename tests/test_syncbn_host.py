"""Host: which normalisation layers spconv_amd/pytorch/norm.py routes to the kernels of csrc/norm.hip, and which of its
two autograd functions a SyncBatchNorm takes (no kernel is launched in this file)."""
import torch
from torch import nn


class _Features:
    """What norm.supported looks at of a feature matrix, without a GPU behind it."""
    is_cuda = True

    def __init__(self, n, C, dtype=torch.float16):
        self.shape, self.dtype = (n, C), dtype

    def dim(self):
        return 2


def test_supported_accepts_exactly_the_two_syncbatchnorm_types():
    import spconv_amd.pytorch as spconv
    from spconv_amd.pytorch import norm
    f = _Features(100, 16)
    assert norm.supported(f, nn.BatchNorm1d(16))
    assert norm.supported(f, nn.SyncBatchNorm(16))
    assert norm.supported(f, spconv.SparseSyncBatchNorm(16))
    assert norm.fused_types() == (nn.BatchNorm1d, nn.SyncBatchNorm, spconv.SparseSyncBatchNorm)

    class Mine(nn.SyncBatchNorm):
        def forward(self, input):
            return super().forward(input) * 2

    class MineSparse(spconv.SparseSyncBatchNorm):
        pass

    assert not norm.supported(f, Mine(16))                     # a subclass with a forward of its own keeps it
    assert not norm.supported(f, MineSparse(16))               # exactly the two types: no other subclass
    assert not norm.supported(f, spconv.SparseBatchNorm(16))   # (as before)
    assert not norm.supported(f, nn.BatchNorm2d(16)) and not norm.supported(f, nn.InstanceNorm1d(16))
    # the existing rules hold for the new types: hooks, channel count, dtype, shape
    hooked = nn.SyncBatchNorm(16)
    hooked.register_forward_hook(lambda m, i, o: None)
    assert not norm.supported(f, hooked)
    assert not norm.supported(f, nn.SyncBatchNorm(32))
    assert not norm.supported(_Features(100, 12), nn.SyncBatchNorm(12))
    assert not norm.supported(_Features(100, 16, torch.float64), nn.SyncBatchNorm(16))
    # without a group to synchronise with, one row in training mode is torch's error, as for BatchNorm1d
    assert not norm.supported(_Features(1, 16), nn.SyncBatchNorm(16))
    assert norm.supported(_Features(1, 16), nn.SyncBatchNorm(16).eval())


def test_switch_restores_torchs_path(monkeypatch):
    from spconv_amd.pytorch import norm
    monkeypatch.setattr(norm, "ENABLED", False)
    assert not norm.supported(_Features(100, 16), nn.SyncBatchNorm(16))


def _record(monkeypatch, norm):
    calls = []
    monkeypatch.setattr(norm._BatchNormFn, "apply", staticmethod(lambda *a: calls.append(("plain", a)) or a[0]))
    monkeypatch.setattr(norm._SyncBatchNormFn, "apply", staticmethod(lambda *a: calls.append(("sync", a)) or a[0]))
    return calls


def test_syncbatchnorm_without_a_process_group_is_the_plain_function(monkeypatch):
    from spconv_amd.pytorch import norm
    calls = _record(monkeypatch, norm)
    x = torch.zeros(10, 8)
    for bn in (nn.SyncBatchNorm(8), nn.SyncBatchNorm(8).eval(), nn.BatchNorm1d(8)):
        assert norm.sync_group(bn) is None
        norm.batch_norm(x, bn)
    assert [c[0] for c in calls] == ["plain"] * 3


def test_syncbatchnorm_in_a_group_takes_the_synchronising_function(monkeypatch):
    """Group sizes as torch.nn.SyncBatchNorm.forward reads them: one rank = nothing to synchronise."""
    from spconv_amd.pytorch import norm
    calls = _record(monkeypatch, norm)
    world = [2]
    monkeypatch.setattr(norm.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(norm.dist, "get_world_size", lambda group=None: world[0])
    x = torch.zeros(10, 8)
    bn = nn.SyncBatchNorm(8)
    assert norm.sync_group(bn) is not None and norm.sync_group(bn)[1] == 2
    assert norm.sync_group(bn.eval()) is None and norm.sync_group(bn, training=True) is not None
    assert norm.sync_group(nn.BatchNorm1d(8)) is None
    bn.train()
    norm.batch_norm(x, bn, relu=True)
    assert calls[-1][0] == "sync" and calls[-1][1][-1] == 2 and calls[-1][1][7] is True
    assert norm.supported(_Features(0, 8), bn) and norm.supported(_Features(1, 8), bn)      # the others have the rows
    assert int(bn.num_batches_tracked) == 1                 # (a host tensor: counted here, as batch_norm() always did)
    norm.batch_norm(x, bn.eval())
    assert calls[-1][0] == "plain"
    world[0] = 1
    norm.batch_norm(x, bn.train())
    assert calls[-1][0] == "plain"
