"""ops.ScratchPool on CPU tensors with explicit stream keys: a buffer handed out for (purpose, device, stream, dtype, size class) is
never replaced - captured hipGraphs hold its address."""
import torch

from aptai_amd import ops


def test_same_key_and_size_class_give_the_same_tensor_and_growth_keeps_the_old_one():
    pool = ops.ScratchPool()
    a = pool.get("sgemm", 100, "cpu", 7)
    assert a.dtype == torch.float32 and a.numel() == 128
    assert pool.get("sgemm", 100, "cpu", 7) is a and pool.get("sgemm", 65, "cpu", 7) is a and pool.get("sgemm", 128, "cpu", 7) is a
    b = pool.get("sgemm", 129, "cpu", 7)                        # a larger request: a new buffer, the old one stays where it is
    assert b is not a and b.numel() == 256
    assert pool.get("sgemm", 100, "cpu", 7) is a and a.data_ptr() != b.data_ptr()
    held = pool.buffers("sgemm")
    assert len(held) == 2 and held[0][1] is a and held[1][1] is b and held[0][0] == 7


def test_size_classes_are_powers_of_two_unless_exact():
    pool = ops.ScratchPool()
    shared = {id(pool.get("colsum", n, "cpu", 0)) for n in range(17, 33)}
    assert len(shared) == 1 and pool.get("colsum", 17, "cpu", 0).numel() == 32
    assert pool.get("colsum", 16, "cpu", 0).numel() == 16 and pool.get("colsum", 1, "cpu", 0) is pool.get("colsum", 16, "cpu", 0)
    e = pool.get("conv", 100, "cpu", None, torch.bfloat16, exact=True)
    assert e.numel() == 100 and e.dtype == torch.bfloat16
    assert pool.get("conv", 101, "cpu", None, torch.bfloat16, exact=True).numel() == 101
    assert pool.get("conv", 100, "cpu", None, torch.bfloat16, exact=True) is e


def test_streams_purposes_and_dtypes_never_share():
    pool = ops.ScratchPool()
    a, b = pool.get("lstm", 64, "cpu", 1, torch.uint8), pool.get("lstm", 64, "cpu", 2, torch.uint8)
    assert a is not b and a.data_ptr() != b.data_ptr()
    assert pool.get("sk", 64, "cpu", 1, torch.uint8) is not a
    assert pool.get("lstm", 64, "cpu", 1, torch.float32) is not a
    assert ops.ScratchPool().get("lstm", 64, "cpu", 1, torch.uint8) is not a              # another pool (a model's own): its own buffers


def test_zero_initialisation_and_listing():
    pool = ops.ScratchPool()
    z = pool.get("lstm", 1000, "cpu", 3, torch.uint8, zero=True)
    assert z.numel() == 1024 and not z.any()
    z[:4] = 1
    assert pool.get("lstm", 1000, "cpu", 3, torch.uint8, zero=True)[:4].all()             # zeroed once, at creation
    big = pool.get("lstm", 5000, "cpu", 3, torch.uint8, zero=True)
    other = pool.get("lstm", 1000, "cpu", 4, torch.uint8, zero=True)
    pool.get("sgemm", 10, "cpu", 3)
    listed = pool.buffers("lstm")
    assert [s for s, _ in listed] == [3, 3, 4] and all(x is y for (_, x), y in zip(listed, (z, big, other)))
    assert len(pool.buffers("lstm", "cpu")) == 3 and pool.buffers("lstm", "cuda:0") == [] and len(pool.buffers("sgemm")) == 1
