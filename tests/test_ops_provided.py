"""CPU: ops._provided -- a caller-provided output is checked as the tensor the op would allocate in its place (device, dtype, contiguity,
leading dims, pitch granule) and raises EsrError otherwise.  The launches that use it: tests/test_gpu_bounds.py."""
import pytest
import torch


def _check(t, like=None, shape=(2, 5, 7), cmin=24, gran=8):
    from ntire2022_esr_amd import ops
    return ops._provided(t, "op: out", torch.empty(0, dtype=torch.bfloat16) if like is None else like, shape, cmin, gran)


def test_a_matching_tensor_is_returned_as_it_is():
    t = torch.zeros(2, 5, 7, 32, dtype=torch.bfloat16)
    assert _check(t) is t
    assert _check(torch.zeros(2, 5, 7, 24, dtype=torch.bfloat16)).shape[-1] == 24         # exactly the channels: the allocated pitch


@pytest.mark.parametrize("bad,word", [
    (lambda: torch.zeros(2, 5, 7, 32, dtype=torch.float16), "dtype"),                     # the op stores bf16
    (lambda: torch.zeros(2, 5, 7, 32, dtype=torch.float32), "dtype"),
    (lambda: torch.zeros(2, 5, 7, 28, dtype=torch.bfloat16), "pitch"),                    # not a multiple of the granule
    (lambda: torch.zeros(2, 5, 7, 16, dtype=torch.bfloat16), "pitch"),                    # does not hold the channels
    (lambda: torch.zeros(2, 5, 8, 32, dtype=torch.bfloat16), "contiguous"),               # another width
    (lambda: torch.zeros(1, 5, 7, 32, dtype=torch.bfloat16), "contiguous"),               # another batch
    (lambda: torch.zeros(2, 5, 7, 64, dtype=torch.bfloat16)[..., :32], "contiguous"),     # a strided slice: the view is (tensor, coff), not a stride
    (lambda: torch.zeros(2, 5, 7, 32, dtype=torch.bfloat16, device="meta"), "tensor on"),  # another device
    (lambda: [[0.0]], "tensor on"),                                                        # not a tensor
])
def test_a_tensor_the_op_would_not_have_allocated_raises(bad, word):
    from ntire2022_esr_amd import _lib as L
    with pytest.raises(L.EsrError, match=word):
        _check(bad())


def test_the_granule_is_the_storage_types():
    from ntire2022_esr_amd import _lib as L
    like = torch.empty(0, dtype=torch.float32)
    assert _check(torch.zeros(2, 5, 7, 28), like, cmin=25, gran=4).shape[-1] == 28        # fp32: granules of 4 channels
    with pytest.raises(L.EsrError, match="pitch"):
        _check(torch.zeros(2, 5, 7, 26), like, cmin=25, gran=4)
