"""Extension.call, the one way modules/_hip.py launches an entry point of the library: what reaches the entry point, what is
refused before it, and what its status becomes.  The entry point is a Python callable entered in the helper's table of
launches, like every entry point of the library, under a name the library does not have and with pointer parameters at
positions 0, 1, 4 and 5: it records its arguments and returns a chosen status.  No kernel is launched."""
import ctypes

import pytest
import torch


class Fake:
    def __init__(self, status=0):
        self.status, self.seen = status, []

    def __call__(self, *args):
        self.seen.append(args)
        return self.status


@pytest.fixture
def fake(monkeypatch):
    from modules import Extension as X
    f = Fake()
    monkeypatch.setitem(X._LAUNCHES, 'mvx_fake', (f, (0, 1, 4, 5)))
    return f


@pytest.mark.gpu
def test_tensors_become_pointers_the_rest_passes_through_and_the_stream_comes_last(fake):
    from modules import Extension as X
    from modules import _hip
    dev = torch.device('cuda', torch.cuda.current_device())
    t = torch.arange(3, dtype=torch.float32, device=dev)
    wide = torch.zeros((4, 6), dtype=torch.float32, device=dev)
    view = wide[:, 2:5]
    assert not view.is_contiguous()
    rest = (None, 7, 0.5, _hip._vptr(view), (ctypes.c_int32 * 3)(1, 2, 3))
    assert isinstance(rest[3], ctypes.c_void_p) and rest[3].value == view.data_ptr() == wide.data_ptr() + 8
    side = torch.cuda.Stream(device=dev)
    assert X.call('mvx_fake', t, *rest) is None
    main_handle = X.raw_stream()
    with torch.cuda.stream(side):
        assert X.call('mvx_fake', t, *rest) is None
        side_handle = X.raw_stream()
    assert side_handle == side.cuda_stream and side_handle != main_handle
    assert main_handle == torch.cuda.current_stream(dev).cuda_stream
    assert len(fake.seen) == 2
    for got, handle in zip(fake.seen, (main_handle, side_handle)):
        assert len(got) == 1 + len(rest) + 1
        assert type(got[0]) is ctypes.c_void_p and got[0].value == t.data_ptr() == X.ptr(t).value
        assert all(g is r for g, r in zip(got[1:-1], rest))                  # the same objects, not copies or conversions
        assert type(got[-1]) is ctypes.c_void_p and (got[-1].value or 0) == handle
    assert fake.seen[0][-1].value == X.stream().value                        # what the helper appends is stream()


@pytest.mark.gpu
def test_a_non_contiguous_device_tensor_is_refused_before_the_call(fake):
    from modules import Extension as X
    t = torch.zeros((4, 6), device='cuda')
    with pytest.raises(X.MvxHipError) as by_ptr:
        X.ptr(t[:, ::2])
    with pytest.raises(X.MvxHipError, match='contiguous') as by_call:
        X.call('mvx_fake', t, t[:, ::2], 3)
    assert str(by_call.value) == str(by_ptr.value)                           # ptr's refusal, in ptr's words
    assert fake.seen == []


def test_a_cpu_tensor_is_refused_before_the_call(fake):
    from modules import Extension as X
    with pytest.raises(X.MvxHipError) as by_ptr:
        X.ptr(torch.zeros(3))
    with pytest.raises(X.MvxHipError, match='device tensors') as by_call:
        X.call('mvx_fake', 3, torch.zeros(3))
    assert str(by_call.value) == str(by_ptr.value)
    assert fake.seen == []


@pytest.mark.gpu                    # the current stream is asked of the device, whatever the callable then returns
@pytest.mark.parametrize('status,text', [(-1, 'mvx_fake failed: argument error -1'), (700, 'mvx_fake failed: hipError_t 700'),
                                         (0, None)])
def test_status_becomes_the_error_text(fake, status, text):
    """The callable is Python: status 700 is a number it returns, no device fault is involved."""
    from modules import Extension as X
    fake.status = status
    if text is None:
        assert X.call('mvx_fake', 1, None, 2, 0.5, None, None) is None
    else:
        with pytest.raises(X.MvxHipError) as e:
            X.call('mvx_fake', 1, None, 2, 0.5, None, None)
        assert str(e.value) == text
    assert len(fake.seen) == 1 and fake.seen[0][:6] == (1, None, 2, 0.5, None, None) and type(fake.seen[0][6]) is ctypes.c_void_p
