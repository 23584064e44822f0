"""Device tensors whose base is float-aligned but not 16-byte aligned, and sentinel-guarded device outputs,
for the C-ABI tests that pass device pointers."""
import numpy as np

GUARD = 32


def offset_view(torch, arr, offset):
    """`arr` (float32 numpy) on the device as a view that starts `offset` elements (0..3) into a fresh flat
    allocation with 3 spare elements. Returns (the view, its allocation, which must stay alive)."""
    arr = np.ascontiguousarray(arr, np.float32)
    flat = torch.full((arr.size + 3,), float("nan"), dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + arr.size].view(arr.shape)
    view.copy_(torch.from_numpy(arr))
    assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + 4 * offset
    assert (view.data_ptr() % 16 != 0) == (offset % 4 != 0)
    return view, flat


def guarded(torch, shape, fill, dtype):
    """(the flat sentinel-filled device buffer, the pointer of its middle part of `shape`)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf.data_ptr() + GUARD * buf.element_size()


def unguard(buf, shape, fill):
    """The middle part as numpy, after checking that the guards on either side still hold `fill`."""
    a = buf.cpu().numpy()
    assert np.all(a[:GUARD] == fill) and np.all(a[-GUARD:] == fill), "a write outside the output"
    return a[GUARD:-GUARD].reshape(shape)
