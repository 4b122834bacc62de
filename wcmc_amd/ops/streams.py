"""The streams a step forks work onto: the weight-gradient side stream, the branch stream of the specular half, and the probe for
two streams that sit on different hardware queues."""
import torch

from .. import ops as _sw          # the package itself: switches and rebound state are read there, when a function runs

_SIDE_STREAMS = {}


def _side_stream(device, of=None):
    """The weight-gradient stream that belongs to stream `of` (default: the CURRENT stream), or None when
    weight gradients should stay on that stream.

    The forked specular branch keeps its weight gradients on its own stream: hipStreamEndCapture (ROCm
    7.0) recurses without end when two forked (non-origin) streams of a capture wait on each other
    (each wait registers the waiter as a child of the other), so only the step's origin stream forks
    and joins a weight-gradient stream."""
    if not _sw.USE_SIDE_STREAM:
        return None
    of = torch.cuda.current_stream(device) if of is None else of
    br = _BRANCH_STREAMS.get((device.type, device.index))
    if br is not None and br.cuda_stream == of.cuda_stream:
        return None
    key = (device.type, device.index, of.cuda_stream)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


# Branch-level concurrency: the diffuse and specular halves of the step (PathNet backbones, KPCN conv
# stacks + kernel apply, their losses and backward passes) are independent until the optimiser.
# Running the specular half on a second stream lets its kernels fill the CUs that the tail of a
# diffuse launch leaves idle (a conv launch is a whole number of 512-workgroup waves); autograd
# replays each half's backward on the stream its forward ran on.
_BRANCH_STREAMS = {}


def branch_stream(device):
    key = (device.type, device.index)
    if key not in _BRANCH_STREAMS:
        _BRANCH_STREAMS[key] = torch.cuda.Stream(device=device)
    return _BRANCH_STREAMS[key]


def _step_streams(device):
    """The streams one step forks work onto from the current stream."""
    device = torch.device(device)
    cur = torch.cuda.current_stream(device)
    out = [_side_stream(device, cur)]
    if _sw.USE_BRANCH_STREAM:
        out.append(branch_stream(device))
    return cur, [s for s in out if s is not None and s.cuda_stream != cur.cuda_stream]


def fork_all_streams(device):
    """Fork every stream the step uses directly from the current stream (under HIP stream capture: make
    them first-level children of the capturing stream before anything else touches them)."""
    if torch.device(device).type != "cuda":
        return
    cur, streams = _step_streams(device)
    for s in streams:
        s.wait_stream(cur)


def join_all_streams(device):
    """Make the current stream wait for every stream the step forked work onto (a stream capture must
    not end with forked work outstanding)."""
    if torch.device(device).type != "cuda":
        return
    cur, streams = _step_streams(device)
    for s in streams:
        cur.wait_stream(s)


# Two streams overlap on the GPU only when the HIP runtime has mapped them onto DIFFERENT hardware queues; it deals its (few) queues
# out to streams as they are created, so two freshly made streams may share one and then run strictly one after the other -- the
# "lottery" of rounds 3-4 (a captured step whose halves ran in series: 13.4 instead of 11.7 ms, decided at stream creation and stable
# for the life of the streams).  ``concurrent_stream_pair`` makes streams until two of them demonstrably run a pair of spin kernels
# side by side, once per device and process; the two-stream step replays its halves on that pair.
_STREAM_PAIRS = {}


def _spin_ms(streams, cycles):
    cur = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for s in streams:
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
    for s in streams:
        cur.wait_stream(s)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def concurrent_stream_pair(device, tries=8):
    """Two side streams of `device` that run concurrently (probed with spin kernels), cached per device; ``.probe`` on the returned
    tuple's first stream holds what was measured (ms of one spin kernel, of the accepted pair, streams tried)."""
    device = torch.device(device)
    key = (device.type, device.index)
    if key in _STREAM_PAIRS:
        return _STREAM_PAIRS[key]
    with torch.cuda.device(device):
        first = torch.cuda.Stream(device=device)
        if not hasattr(torch.cuda, "_sleep"):                # (no spin kernel to probe with: two fresh streams, unprobed)
            pair = (first, torch.cuda.Stream(device=device))
            pair[0].probe = {"spin_ms": None, "pair_ms": None, "streams_tried": 2, "concurrent": None}
            _STREAM_PAIRS[key] = pair
            return pair
        cycles = 200000
        one = _spin_ms([first], cycles)
        one = _spin_ms([first], cycles)                      # (second run: without first-launch costs)
        if one < 0.2:                                        # aim at ~0.3 ms per spin: long against launch latencies
            cycles = int(cycles * 0.3 / max(one, 1e-3))
            one = _spin_ms([first], cycles)
        pool, best = [first], None
        for _ in range(tries):
            cand = torch.cuda.Stream(device=device)
            for other in pool:
                t = min(_spin_ms([other, cand], cycles), _spin_ms([other, cand], cycles))
                if best is None or t < best[0]:
                    best = (t, other, cand)
                if t < 1.4 * one:
                    break
            pool.append(cand)
            if best[0] < 1.4 * one:
                break
    pair = (best[1], best[2])
    pair[0].probe = {"spin_ms": round(one, 4), "pair_ms": round(best[0], 4), "streams_tried": len(pool), "concurrent": bool(best[0] < 1.4 * one)}
    _STREAM_PAIRS[key] = pair
    return pair


class on_branch:
    """``with on_branch(device) as br: y = f(x)`` runs f on the branch stream after everything enqueued
    so far on the current stream; ``br.join(y, ...)`` makes the current stream wait for it."""

    def __init__(self, device):
        self.enabled = _sw.USE_BRANCH_STREAM and torch.device(device).type == "cuda"
        if self.enabled:
            self.main = torch.cuda.current_stream(device)
            self.stream = branch_stream(torch.device(device))
            self.ctx = torch.cuda.stream(self.stream)

    def __enter__(self):
        if self.enabled:
            self.stream.wait_stream(self.main)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.enabled:
            self.ctx.__exit__(*exc)
        return False

    def join(self, *tensors):
        if self.enabled:
            self.main.wait_stream(self.stream)
            for t in tensors:
                if isinstance(t, torch.Tensor):
                    t.record_stream(self.main)
