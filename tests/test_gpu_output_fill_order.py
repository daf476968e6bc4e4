"""An output tensor that a Scene / InstancedScene method allocates itself is FILLED (misses are +inf / 0) before the launch writes the hits into
it.  torch enqueues that fill on the current stream; when the launch goes to another stream the fill has to go there too, or it can land after the
kernel and wipe the frame (what happens as soon as the current stream is busy).  Here the current stream is kept busy for 3 ms by the workbench
library's stream-ordered pause while frames are traced on a second stream; they must equal the frames of the idle device."""
import numpy as np
import pytest

from tests.test_bvh_fast_host import soup

pytestmark = pytest.mark.gpu


def test_outputs_allocated_by_the_binding_are_filled_on_the_launch_stream():
    import torch
    from snail_amd import _lib, survey_camera
    from snail_amd.instances import InstancedScene
    from snail_amd.scene import Scene
    tv = soup(1000, 31)
    cam = survey_camera(tv)
    sc = Scene.from_fast(tv, 0)
    isc = InstancedScene([sc], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), dtype=np.float32), np.zeros(1, dtype=np.int32))
    lo, hi = tv.reshape(-1, 3).min(axis=0), tv.reshape(-1, 3).max(axis=0)
    lights = np.array([[(lo[0] + hi[0]) / 2, hi[1] + 5.0, (lo[2] + hi[2]) / 2, 1.0, 0.9, 0.8, 4.0 * float((hi - lo).max())]], dtype=np.float32)

    def frames(stream):
        f = sc.trace_primary(cam, 256, 256, stream=stream)
        img = sc.render_whitted(cam, 256, 256, lights, stream=stream)
        inst = isc.trace_primary(cam, 256, 256, stream=stream)
        return [f.t, f.tri_id, img, inst[0], inst[4]]

    want = [x.cpu().numpy().copy() for x in frames(None)]
    assert np.isfinite(want[0]).sum() > 1000 and (want[2] != 0).any()          # hits, and a lit image: a wiped frame differs
    pause = _lib.debug_lib().snail_debug_delay_dev
    # several second streams in turn: which hardware queue a stream shares with the current one depends on how many were used before it
    for k in range(5):
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert pause(3000.0, None) == 0, _lib.debug_lib().snail_last_error()    # the current (default) stream is busy for 3 ms ...
        got = frames(side)                                                      # ... while these are traced on another
        torch.cuda.synchronize()
        for name, a, b in zip(("t", "triId", "lit image", "instanced t", "instanced triId"), got, want):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8)), (name, k)
    isc.close(); sc.close()
