"""What the device post-processing path needs that can be checked without a GPU: the entry point refuses a null handle, the
pool of page-locked output blocks never hands out a block that is still viewed, and the drivers fall back to the host path."""
import ctypes as C
import gc

import numpy as np

from general_motion_retargeting_amd import _lib, dataset


def test_null_handle_is_an_argument_error():
    L = _lib.lib()
    src = (_lib.PostSrc * 1)(_lib.PostSrc(1, 1, None, None))
    rc = L.gmr_postprocess_clips_dev(None, C.cast(src, C.c_void_p), 1, 36, None, 1, 1, 3, 0.0, None, None, None, None, None, None)
    assert rc == -1 and b"null fk handle" in L.gmr_last_error()


class _Block:
    """stand-in for a page-locked allocation: ordinary memory behind the same two attributes"""
    made = []

    def __init__(self, nbytes):
        self._mem = C.create_string_buffer(int(nbytes))
        self.ptr, self.nbytes = C.c_void_p(C.addressof(self._mem)), int(nbytes)
        _Block.made.append(self)


def test_a_block_returns_to_the_pool_only_when_its_last_view_is_dropped():
    _Block.made.clear()
    pool = dataset.PinnedPool(alloc=_Block)
    buf = pool.take(1000)
    a = np.frombuffer(buf, dtype=np.float64, count=50, offset=0).reshape(10, 5)
    b = np.frombuffer(buf, dtype=np.float32, count=20, offset=400)
    row = a[3:7]                                    # what a motion dict holds: a view of a view
    a[:] = 1.5
    del buf, a
    gc.collect()
    assert pool.free_blocks == 0 and pool.blocks_allocated == 1
    other = pool.take(900)                          # the first block is still viewed: a batch gets another one
    assert pool.blocks_allocated == 2 and len(_Block.made) == 2
    np.frombuffer(other, dtype=np.uint8)[:] = 0
    assert (row == 1.5).all()                       # ... and writing it leaves the kept rows alone
    del b
    gc.collect()
    assert pool.free_blocks == 0
    del row
    gc.collect()
    assert pool.free_blocks == 1
    again = pool.take(1000)                         # the freed block serves the next batch; nothing new is allocated
    assert pool.blocks_allocated == 2 and C.addressof(again) == _Block.made[0].ptr.value
    big = pool.take(10 ** 6)                        # no free block is large enough: a new one
    assert pool.blocks_allocated == 3 and big is not None
    del other, again, big
    gc.collect()
    assert pool.free_blocks == 3


def test_the_pool_keeps_a_bounded_number_of_free_blocks():
    pool = dataset.PinnedPool(alloc=_Block, keep=2)
    bufs = [pool.take(64) for _ in range(5)]
    assert pool.blocks_allocated == 5
    del bufs
    gc.collect()
    assert pool.free_blocks == 2


def test_host_path_is_selected_by_the_switch_and_without_a_gpu(monkeypatch):
    class _Lib:
        def __init__(self, n):
            self.n = n

        def gmr_device_count(self):
            return self.n

    monkeypatch.setattr(_lib, "lib", lambda: _Lib(1))
    monkeypatch.delenv("GMR_DATASET_POST", raising=False)
    assert dataset.post_path() == "device"
    monkeypatch.setenv("GMR_DATASET_POST", "host")
    assert dataset.post_path() == "host"
    monkeypatch.setenv("GMR_DATASET_POST", "device")
    monkeypatch.setattr(_lib, "lib", lambda: _Lib(0))
    assert dataset.post_path() == "host"

    def missing():
        raise _lib.GmrHipError("not built")
    monkeypatch.setattr(_lib, "lib", missing)
    assert dataset.post_path() == "host"


def test_finish_takes_the_host_path_when_told_to(monkeypatch):
    """ClipRetargeter.finish with stand-ins for the GPU calls: with GMR_DATASET_POST=host the batch goes through
    retarget_group + postprocess_clips, never through the device path"""
    calls = []
    rt = dataset.ClipRetargeter.__new__(dataset.ClipRetargeter)

    class _Sol:
        nq, nhuman = 36, 3

    class _Gmr:
        hip_solver = _Sol()
        xml_file = "unused"

        class model:
            qpos0 = np.zeros(36)

        def _flags(self, g):
            return 0

    rt.gmr, rt.height_adjust, rt.root_origin_offset, rt.offset_to_ground = _Gmr(), True, True, False
    rt._km, rt._pin, rt._dev_post, rt.timing = object(), {}, None, {}
    monkeypatch.setattr(rt, "_buf", lambda name, shape, dtype: np.zeros(shape, dtype))
    monkeypatch.setattr(rt, "_finish_device", lambda fps, lens: calls.append("device") or [])
    monkeypatch.setattr(_lib, "retarget_group", lambda jobs, flags, slices, outs=None: calls.append("group") or outs)
    monkeypatch.setattr(dataset, "postprocess_clips", lambda q, km, fps, h, o: calls.append("host") or [{"n": len(x)} for x in q])
    monkeypatch.setattr(dataset, "post_path", lambda: "host")
    rt.begin(4, 2, 100)
    assert rt.add(np.zeros((4, 3, 7))) and rt.add(np.zeros((2, 3, 7)))
    assert rt.finish([30, 30]) == [{"n": 4}, {"n": 2}] and calls == ["group", "host"]
    monkeypatch.setattr(dataset, "post_path", lambda: "device")
    rt.begin(4, 2, 100)
    assert rt.add(np.zeros((4, 3, 7)))
    rt.finish([30])
    assert calls == ["group", "host", "device"]
