"""Frames for ``wcmc_amd.denoise``, streamed to the device in row bands and prefetched one frame ahead.

A raw frame is (H, W, S, 104) floats -- 3.1 GB at 1280 x 720 x 8 spp, 55 GB at 1920 x 1080 x 64 spp -- and the network needs none of
it: only ``kpcn`` (H, W, 44) and ``llpm`` (H, W, S, 37).  Everything the two preprocessing functions compute is per pixel, except the
image maximum of the mean depth and the backward differences, and both of those belong to the finish pass of
``ops.preprocess_kpcn_begin / _rows / _end``.  So the frame never lies whole anywhere but on disk:

  * ``BandReader``: ``workers`` threads copy row bands of the memory-mapped parts (``denoise.read_raw``: the file and its continuation
    files) straight into a ring of ``workers + 2`` pinned slots of ONE band each -- one host copy per byte, the conversion to float32
    included -- and hand the bands out in row order;
  * ``FrameStreamer``: a producer thread sends each band through ONE copy stream -- the host-to-device copy into the device band
    buffer, ``sanitize_``, ``preprocess_kpcn_rows``, ``preprocess_llpm(out=rows)`` -- closes the frame with ``preprocess_kpcn_end`` and
    hands ``(kpcn, llpm)`` over behind an event, as ``loader.ImageStager`` hands its buffers over.  It runs one frame ahead of the
    consumer: frame n + 1 crosses PCIe while the network runs frame n and the host writes its files.

For an SBMC / LBMC model (``base_model='sbmc' | 'lbmc'``) the same threads, stream and ring produce ``(sbmc_s, sbmc_p or None, llpm)``:
every buffer is per sample, so a band is final when ``preprocess_sbmc`` and ``preprocess_llpm`` have run on it.

``loader.py`` stages whole images for training and stays as it is; its stop-flag queue idiom (``ImageStager._get`` / ``_put``) is
reused here.  ``scripts/time_denoise_stream.py`` measures the route against ``denoise.upload_raw``.
"""
import collections
import math
import queue
import threading

import numpy as np
import torch

from .loader import ImageStager

RAW_C = 104                                          # channels of renderer output (denoise._open_raw)
BAND_TARGET_BYTES = 64 << 20                         # of one band, when the caller names no band height: DESIGN.md section 16


def band_ranges(h, band_rows):
    """The ``(row0, rows)`` partition of the rows ``[0, h)`` into bands of ``band_rows`` (the last one may be shorter)."""
    h, band_rows = int(h), int(band_rows)
    if h < 1:
        raise ValueError("band_ranges: a frame has at least one row, got %d" % h)
    if band_rows < 1:
        raise ValueError("band_rows should be at least 1, got %d" % band_rows)
    return [(r0, min(band_rows, h - r0)) for r0 in range(0, h, band_rows)]


def default_band_rows(h, w, spp, target_bytes=BAND_TARGET_BYTES):
    """Rows of a band of about ``target_bytes`` of float32 raw samples, between one row and the frame."""
    return max(1, min(int(h), int(target_bytes) // (int(w) * int(spp) * RAW_C * 4)))


_COPY_STREAMS = {}


def copy_stream(device):
    """THE copy stream of ``device``: one per device and process, shared by every ``FrameStreamer`` (as ``ops.branch_stream`` is the one
    branch stream).  A stream per streamer would draw a new one from torch's pool of 32 for every frame sequence: the pool hands the
    same streams out again after 32 draws, and every stream used for the first time takes a place in the runtime's dealing of its four
    hardware queues, which moves the streams a later hipGraph capture forks onto.  One streamer at a time uses it; two would share it
    and run one behind the other, which is still correct."""
    device = torch.device(device)
    key = (device.type, device.index)
    if key not in _COPY_STREAMS:
        _COPY_STREAMS[key] = torch.cuda.Stream(device=device)
    return _COPY_STREAMS[key]


class _AnyStop:
    """``is_set()`` over several events: what ``ImageStager._get`` polls."""

    def __init__(self, *events):
        self.events = events

    def is_set(self):
        return any(e.is_set() for e in self.events)


class PinnedRing:
    """``n`` host staging slots, each one flat float32 buffer that grows to the largest band it has held (pinned with ``pin``).  A
    slot goes back with the event of the host-to-device copy out of it; whoever takes it next waits for that event first."""

    def __init__(self, n, pin):
        self.pin, self.peak_nbytes = bool(pin), 0                     # (the most the ring has held at once)
        self.slots = [{'buf': None, 'event': None} for _ in range(int(n))]
        self.free_q = queue.Queue()
        for s in self.slots:
            self.free_q.put(s)

    def take(self, stop):
        slot = ImageStager._get(self.free_q, stop)
        if slot is not None and slot['event'] is not None:
            slot['event'].synchronize()                               # (the previous host -> device copy out of this slot)
            slot['event'] = None
        return slot

    def release(self, slot, event=None):
        slot['event'] = event
        self.free_q.put(slot)

    def view(self, slot, shape):
        n = math.prod(shape)
        if slot['buf'] is None or slot['buf'].numel() < n:
            slot['buf'] = None
            slot['buf'] = torch.empty(n, dtype=torch.float32, pin_memory=self.pin)
            self.peak_nbytes = max(self.peak_nbytes, self.nbytes())
        return slot['buf'][:n].view(shape)

    def nbytes(self):
        return sum(s['buf'].numel() * 4 for s in self.slots if s['buf'] is not None)

    def clear(self):
        """Give the slots' memory back (after the copies out of them); ``peak_nbytes`` keeps what the ring held."""
        for s in self.slots:
            if s['event'] is not None:
                s['event'].synchronize()
            s['buf'], s['event'] = None, None


class BandReader:
    """Iterate the row bands of one frame as ``(slot, row0, rows)``, in row order: ``ring.view(slot, (rows, W, spp, 104))`` holds the
    float32 samples of frame rows ``[row0, row0 + rows)``; give the slot back with ``ring.release(slot, event)``.

    ``parts`` are ``denoise.read_raw``'s: ``[(H, W, s_k, 104)]`` array-likes (memory maps; anything with ``shape`` and row slicing),
    whose samples lie side by side along axis 2 of the frame.  ``workers`` threads each take a free slot and write every part's rows
    at its sample offset of the slot with one ``np.copyto`` from the mapped file -- the only host copy, and the conversion that
    ``np.array(part, dtype=np.float32)`` makes; numpy releases the interpreter lock for it, so the threads' page-cache reads overlap
    each other and the consumer's DMA.  Whatever order they finish in, bands leave in row order, and an error of band k reaches the
    consumer when band k is due.  The ring holds ``workers + 2`` slots (one per worker, one in the consumer's hands, one whose copy
    is still in flight); nothing of the frame's size is allocated.  No GPU call in here with ``pin=False``."""

    def __init__(self, parts, band_rows, workers=4, pin=None, ring=None, stop=None):
        self.parts = list(parts)
        h, w = self.parts[0].shape[:2]
        for p in self.parts:
            if len(p.shape) != 4 or tuple(p.shape[:2]) != (h, w) or p.shape[3] != RAW_C or p.shape[2] < 1:
                raise ValueError("BandReader: the parts should be (%d, %d, s_k, %d), got %s" % (h, w, RAW_C, tuple(p.shape)))
        self.h, self.w, self.spp = h, w, sum(p.shape[2] for p in self.parts)
        self.ranges = band_ranges(h, band_rows)
        self.workers = max(1, int(workers))
        if ring is None:
            ring = PinnedRing(self.workers + 2, torch.cuda.is_available() if pin is None else pin)
        self.ring = ring
        self.done = threading.Event()                                 # this frame's readers; `stop` is the owner's flag
        self.stop = _AnyStop(self.done) if stop is None else _AnyStop(self.done, stop)

    def _load(self, row0, rows):
        slot = self.ring.take(self.stop)
        if slot is None:
            return None
        try:
            dst = self.ring.view(slot, (rows, self.w, self.spp, RAW_C)).numpy()
            s0 = 0
            for p in self.parts:
                np.copyto(dst[:, :, s0:s0 + p.shape[2]], p[row0:row0 + rows], casting='unsafe')
                s0 += p.shape[2]
        except BaseException:
            self.ring.release(slot)
            raise
        return slot, row0, rows

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="wcmc-band")
        pending, it = collections.deque(), iter(self.ranges)
        try:
            for rng in self.ranges[:self.workers]:
                pending.append(pool.submit(self._load, *next(it)))
            while pending:
                res = pending.popleft().result()                      # in row order; reader errors surface here
                nxt = next(it, None)
                if nxt is not None and not self.stop.is_set():
                    pending.append(pool.submit(self._load, *nxt))
                if res is None:
                    return
                yield res
        finally:
            self.done.set()
            for f in pending:
                f.cancel()
            pool.shutdown(wait=True)
            for f in pending:                                         # bands read but never handed out: their slots go back
                if f.done() and not f.cancelled() and f.exception() is None and f.result() is not None:
                    self.ring.release(f.result()[0])


class _FrameStream:
    """The state and the two threads' code behind ``FrameStreamer``.  Neither the producer thread nor the consumer's generator holds
    the ``FrameStreamer`` itself, so dropping that one ends them."""

    def __init__(self, files, spp, device, band_rows=None, workers=4, max_depth=5, target_bytes=BAND_TARGET_BYTES,
                 base_model='kpcn', use_sbmc_buf=True):
        from .datasets import sample_flags
        if band_rows is not None and int(band_rows) < 1:
            raise ValueError("band_rows should be at least 1, got %d" % band_rows)
        self.base_model, _, self.use_sbmc_buf = sample_flags(base_model, True, use_sbmc_buf)     # ('lbmc': 'sbmc' without sbmc_p)
        self.files, self.spp = list(files), spp
        self.band_rows = None if band_rows is None else int(band_rows)
        self.workers, self.max_depth, self.target_bytes = max(1, int(workers)), max_depth, int(target_bytes)
        self.device = torch.device(device)
        if self.device.index is None:                                 # 'cuda' -> the current device, by index (threads need it)
            self.device = torch.device(self.device.type, torch.cuda.current_device())
        self.copy_stream = copy_stream(self.device)
        self.ring, self.finish_events, self.bytes_moved = None, None, 0
        self._band = None                                             # the device band buffer (flat)
        self._scratch_p = None                                        # sample-based without sbmc_p: one band's unread out_p (flat)

    def _frame(self, fn, ring, stop):
        """Enqueue one frame on the copy stream; ``(buffers, before_end, after_end)`` or None when the consumer has gone.  THE band
        loop, for every model family: what differs between them is in ``_kpcn_family`` / ``_sample_family``."""
        from .. import ops
        from ..denoise import read_raw
        parts, spp = read_raw(fn, self.spp)
        h, w = parts[0].shape[:2]
        band_rows = min(h, self.band_rows or default_band_rows(h, w, spp, self.target_bytes))
        reader = BandReader(parts, band_rows, self.workers, ring=ring, stop=stop)
        bands, seen = iter(reader), 0
        try:
            with torch.cuda.stream(self.copy_stream):
                family = self._kpcn_family if self.base_model == 'kpcn' else self._sample_family
                bufs, on_band, end = family(h, w, spp, band_rows)
                band = self._flat('_band', band_rows * w * spp * RAW_C)
                for slot, row0, rows in bands:
                    shape = (rows, w, spp, RAW_C)
                    d_band = band[:math.prod(shape)].view(shape)
                    d_band.copy_(ring.view(slot, shape), non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(self.copy_stream)
                    ring.release(slot, ev)                            # (the event guards the pinned slot's reuse)
                    ops.sanitize_(d_band)
                    on_band(d_band, row0, rows)
                    self.bytes_moved += d_band.numel() * 4
                    seen += 1
                if seen < len(reader.ranges):                         # the reader gave up: the stop flag is set
                    return None
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record(self.copy_stream)
                if end is not None:                                   # (no finish pass: the pair brackets nothing)
                    end()
                ev1.record(self.copy_stream)
        finally:
            bands.close()
        return bufs, ev0, ev1

    def _flat(self, name, n):
        """The flat device buffer ``self.<name>``, grown to at least ``n`` floats.  The old one is dropped before the new one is
        allocated: it is used on the copy stream alone, so the allocator may reuse it at once."""
        if getattr(self, name) is None or getattr(self, name).numel() < n:
            setattr(self, name, None)
            setattr(self, name, torch.empty(n, device=self.device, dtype=torch.float32))
        return getattr(self, name)

    # What a model family supplies to ``_frame``, called on the copy stream for a frame of (h, w, spp) in bands of ``band_rows``: it
    # allocates the frame's buffers and returns ``(buffers, on_band(d_band, row0, rows), end() or None)`` -- what to run on one sanitised
    # band, and what closes the frame between the two timing events.
    def _kpcn_family(self, h, w, spp, band_rows):
        """``(kpcn, llpm)``: the statistics of a band go to the (h, w) workspace, ``preprocess_kpcn_end`` closes the frame."""
        from .. import ops
        kpcn, ws = ops.preprocess_kpcn_begin(h, w, self.device)
        llpm = torch.empty((h, w, spp, 7 + 5 * (self.max_depth + 1)), device=self.device, dtype=torch.float32)

        def on_band(d_band, row0, rows):
            ops.preprocess_kpcn_rows(d_band, row0, kpcn, ws, self.max_depth)
            ops.preprocess_llpm(d_band, self.max_depth, out=llpm[row0:row0 + rows])
        return (kpcn, llpm), on_band, lambda: ops.preprocess_kpcn_end(kpcn, ws, spp)

    def _sample_family(self, h, w, spp, band_rows):
        """``(sbmc_s, sbmc_p or None, llpm)``.  Every buffer is per sample, so a band is final when its kernels have run: no begin /
        end, no workspace.  ``wcmc_preprocess_sbmc`` writes both of its outputs; without ``use_sbmc_buf`` the second goes to a
        band-sized scratch that the next band overwrites."""
        from .. import ops
        pc = 11 * (self.max_depth + 1)
        new = lambda c: torch.empty((h, w, spp, c), device=self.device, dtype=torch.float32)   # noqa: E731
        sbmc_s, llpm = new(27), new(7 + 5 * (self.max_depth + 1))
        sbmc_p = new(pc) if self.use_sbmc_buf else None
        scratch = None if self.use_sbmc_buf else self._flat('_scratch_p', band_rows * w * spp * pc)

        def on_band(d_band, row0, rows):
            out_p = sbmc_p[row0:row0 + rows] if self.use_sbmc_buf else scratch[:rows * w * spp * pc].view(rows, w, spp, pc)
            ops.preprocess_sbmc(d_band, self.max_depth, out_s=sbmc_s[row0:row0 + rows], out_p=out_p)
            ops.preprocess_llpm(d_band, self.max_depth, out=llpm[row0:row0 + rows])
        return (sbmc_s, sbmc_p, llpm), on_band, None

    def _produce(self, out_q, permits, stop):
        try:
            torch.cuda.set_device(self.device)
            self.ring = ring = PinnedRing(self.workers + 2, pin=True)
            for fn in self.files:
                while not permits.acquire(timeout=0.2):               # a third frame's buffers wait for the first one's to go
                    if stop.is_set():
                        return
                got = self._frame(fn, ring, stop)
                if got is None or not ImageStager._put(out_q, got, stop):
                    return
                del got
            ImageStager._put(out_q, None, stop)
        except BaseException as exc:                                  # surface reader / device errors in the consumer
            ImageStager._put(out_q, exc, stop)
        finally:
            self._band = self._scratch_p = None

    def _consume(self):
        out_q, stop, permits = queue.Queue(maxsize=1), threading.Event(), threading.Semaphore(2)
        worker = threading.Thread(target=self._produce, args=(out_q, permits, stop), daemon=True, name="wcmc-frame-streamer")
        worker.start()
        try:
            while True:
                got = out_q.get()
                if got is None:
                    return
                if isinstance(got, BaseException):
                    exc, got = got, None                              # (no local keeps the exception: its traceback holds this frame)
                    try:
                        raise exc
                    finally:
                        del exc
                bufs, ev0, ev1 = got
                del got
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev1)                                   # the consumer's stream, not the host, waits
                for t in bufs:
                    if t is not None:
                        t.record_stream(cur)
                self.finish_events = (ev0, ev1)
                yield bufs
                del bufs, t
                permits.release()
        finally:
            stop.set()                                                # the producer's and the readers' queue waits poll this flag
            try:
                while True:
                    out_q.get_nowait()
            except queue.Empty:
                pass
            worker.join(timeout=5.0)
            if self.ring is not None and not worker.is_alive():
                self.ring.clear()                                     # the pinned memory goes back here, not whenever the streamer is collected


class FrameStreamer:
    """An iterator over the device buffers ``(kpcn (H, W, 44), llpm (H, W, S, 37))`` of the frames ``files``, in order, each bit for bit
    what ``denoise.upload_raw`` + ``DenoisePreprocessor._preprocess_kpcn / _preprocess_llpm`` give for the frame.  One pass: the threads
    start with the first ``next()``.

    Per frame a producer thread opens the parts (``denoise.read_raw(fn, spp)``), allocates the two buffers and the workspace, and for
    each band of ``BandReader``, on the ONE copy stream and in this order: the asynchronous host-to-device copy out of the pinned slot
    into the device band buffer, ``ops.sanitize_``, ``ops.preprocess_kpcn_rows``, ``ops.preprocess_llpm(out=rows)``; after the last
    band ``ops.preprocess_kpcn_end``.  There is no copy / compute overlap inside a frame (the kernels are half a percent of the
    copy); the reader threads overlap the page-cache reads with the DMA.  The buffers are handed over behind an event: the
    consumer's current stream waits for it, ``record_stream`` is called, and a pinned slot is reused only after its copy's event.

    The producer runs one frame ahead and no further: at most two frames' buffers are alive, the consumer's and the next one's
    (the consumer's count ends when it asks for the next frame, so it should have dropped its references by then).  Device memory
    besides: one band and the (H, W) workspace; pinned host memory: ``workers + 2`` bands.  ``band_rows=None`` takes
    ``default_band_rows`` of each frame; a number is a memory control, never another route.

    ``base_model='sbmc'`` / ``'lbmc'``: the frames of the sample-based models, ``(sbmc_s (H, W, S, 27), sbmc_p (H, W, S, 66) or None,
    llpm)`` -- each band through ``ops.sanitize_``, ``ops.preprocess_sbmc(out_s=rows, out_p=rows)`` and ``ops.preprocess_llpm(out=rows)``
    on the same stream, pinned ring and one-frame-ahead rule; everything is per sample, so there is no workspace and no finish pass.
    ``sbmc_p`` exists only for 'sbmc' with ``use_sbmc_buf`` (otherwise the kernel's second output goes to one band of scratch).

    ``finish_events``: the timing events around the last frame's ``preprocess_kpcn_end``; ``ring``: the pinned ring, once the first
    band has been read.  Reader and device errors are raised in the consumer; a consumer that leaves early (``break``, an exception,
    ``close()``) stops the threads and releases the ring."""

    def __init__(self, files, spp, device, band_rows=None, workers=4, max_depth=5, target_bytes=BAND_TARGET_BYTES,
                 base_model='kpcn', use_sbmc_buf=True):
        self._stream = _FrameStream(files, spp, device, band_rows, workers, max_depth, target_bytes, base_model, use_sbmc_buf)
        self._frames = None                                           # the consumer's generator, from the first next()

    finish_events = property(lambda self: self._stream.finish_events)
    ring = property(lambda self: self._stream.ring)
    bytes_moved = property(lambda self: self._stream.bytes_moved)
    copy_stream = property(lambda self: self._stream.copy_stream)

    def __iter__(self):
        return self

    def __next__(self):
        if self._frames is None:
            self._frames = self._stream._consume()
        return next(self._frames)

    def close(self):
        """Stop the threads and release the ring: what leaving the iteration early ends in, at the latest when the streamer goes."""
        if self._frames is None:
            self._frames = iter(())                                   # never started: nothing to start any more
        else:
            self._frames.close()

    def __del__(self):
        try:
            self.close()
        except Exception:                                             # (interpreter shutdown: nothing left to stop)
            pass
