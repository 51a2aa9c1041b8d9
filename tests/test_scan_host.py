"""CPU: every refusal of the selective scan, the causal convolution and SerializedMamba (spconv_amd/pytorch/_scan.py)
comes with its message before the library is called (nothing here touches a GPU)."""
import pytest
import torch

import spconv_amd.pytorch as spconv
from spconv_amd.pytorch import functional as F

N = 8


def scan_args(Dm=64, G=1, states=16, dtype=torch.float16, **over):
    seq = F.scan_sequences(offsets=torch.tensor([0, N], dtype=torch.int32), n=N)
    a = dict(u=torch.zeros((N, Dm), dtype=dtype), delta=torch.zeros((N, Dm), dtype=dtype), A=torch.zeros((Dm, states)),
             B=torch.zeros((N, G, states), dtype=dtype), C=torch.zeros((N, G, states), dtype=dtype), seq=seq)
    a.update(over)
    return a


@pytest.mark.parametrize("kw,exc,word", [
    (dict(states=8), NotImplementedError, "d_state must be 16"),
    (dict(Dm=96), NotImplementedError, "Dm must be a multiple of 64"),
    (dict(Dm=2112), NotImplementedError, "at most 2048"),
    (dict(Dm=128, G=4), NotImplementedError, "G must divide Dm into multiples of 64"),
    (dict(Dm=192, G=2), NotImplementedError, "G must divide Dm into multiples of 64"),
    (dict(dtype=torch.float64), NotImplementedError, "float16, bfloat16 or float32"),
    (dict(delta=torch.zeros((N, 64))), ValueError, "delta is .*nothing is cast"),
    (dict(A=torch.zeros((64, 16), dtype=torch.complex64)), NotImplementedError, "complex A"),
    (dict(D=torch.zeros(64, dtype=torch.float16)), ValueError, "D is float32"),
    (dict(seq=F.scan_sequences(offsets=torch.tensor([0, 4], dtype=torch.int32), n=4)), ValueError, "name 4 rows"),
    (dict(), NotImplementedError, "no CPU path"),
])
def test_scan_refusals(kw, exc, word, monkeypatch):
    monkeypatch.setattr("spconv_amd._lib.load", lambda: pytest.fail("the library was called"))
    shape = {k: kw.pop(k) for k in ("Dm", "G", "states", "dtype") if k in kw}
    with pytest.raises(exc, match=word):
        F.selective_scan(**scan_args(**shape, **kw))


@pytest.mark.parametrize("kw,exc,word", [
    (dict(weight=torch.zeros((64, 5))), NotImplementedError, "width must be in 2 .. 4"),
    (dict(weight=torch.zeros((64, 1))), NotImplementedError, "width must be in 2 .. 4"),
    (dict(x=torch.zeros((N, 32))), NotImplementedError, "Dm must be a multiple of 64"),
    (dict(activation="relu"), NotImplementedError, "None or 'silu'"),
    (dict(weight=torch.zeros((64, 4), dtype=torch.bfloat16)), ValueError, "weight is .* or float32"),
    (dict(x=torch.zeros((N, 64), dtype=torch.float64)), NotImplementedError, "float16, bfloat16 or float32"),
])
def test_convolution_refusals(kw, exc, word, monkeypatch):
    monkeypatch.setattr("spconv_amd._lib.load", lambda: pytest.fail("the library was called"))
    a = dict(x=torch.zeros((N, 64), dtype=torch.float16), weight=torch.zeros((64, 4)),
             seq=F.scan_sequences(offsets=torch.tensor([0, N], dtype=torch.int32), n=N))
    a.update(kw)
    with pytest.raises(exc, match=word):
        F.causal_conv1d_rows(**a)


def test_sequences_and_module_refusals():
    with pytest.raises(ValueError, match="contiguous int32 tensor"):
        F.scan_sequences(offsets=torch.tensor([0, N]), n=N)
    with pytest.raises(ValueError, match="give n"):
        F.scan_sequences(offsets=torch.tensor([0, N], dtype=torch.int32))
    seq = F.scan_sequences(offsets=torch.tensor([0, 3, N], dtype=torch.int32), order=torch.arange(N, dtype=torch.int32))
    assert (seq.num_sequences, seq.n) == (2, N)
    for kw, word in ((dict(d_state=8), "d_state must be 16"), (dict(d_conv=5), "d_conv must be in 2 .. 4"),
                     (dict(d_model=48), "multiple of 64"), (dict(d_model=2048), "at most 2048")):
        with pytest.raises(NotImplementedError, match=word):
            spconv.SerializedMamba(**{"d_model": 64, **kw})
