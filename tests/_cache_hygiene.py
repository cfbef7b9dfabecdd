"""What a GPU test module that fills device memory with random bytes does when it is done (tests/test_augment_gpu.py,
tests/test_spatial_gpu.py).  A helper module (like tests/_guarded.py), not a test file."""
import gc

import torch


def hand_the_cache_back_zeroed(dev) -> None:
    """Leave the caching allocator as the rest of the suite has always found it (tests/_guarded.py zero-fills its buffers for the
    same reason): a module's freed blocks hold random image bytes, and later tests of the suite compare two runs of kernels bit for
    bit.  Every inactive block of the cache is claimed at its own size, largest first, zero-filled and released; twice, for the
    fragments the first round split."""
    gc.collect()
    torch.cuda.synchronize()
    for _ in range(2):
        held = []
        for seg in torch.cuda.memory_snapshot():
            for b in seg["blocks"]:
                if b["state"] == "inactive":
                    held.append((b["size"], seg["segment_type"]))
        held.sort(reverse=True)
        keep = []
        for size, kind in held:
            for n in ([size] if kind == "large" or size <= (1 << 20) else [1 << 20, size - (1 << 20)]):   # a small-pool request is <= 1 MiB
                keep.append(torch.zeros(n, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        del keep
