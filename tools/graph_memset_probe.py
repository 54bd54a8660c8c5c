"""Does a HIP graph replay the memset nodes of captured hipMemsetAsync calls?  No libdpr in it: ctypes on the HIP
runtime that torch has loaded, torch.cuda.graph for the capture.

Six buffers of 27, 9, 3, 6, 8 and 9003 floats (the sizes of the channel pullback's six clears) are filled with NaN,
a graph of six hipMemsetAsync(ptr, 0, bytes) and one kernel is replayed, and the words that are not zero afterwards
are counted, with the last four words of each buffer in hex.  From the third replay on some host-to-device copies run
between the replays.  The output of one MI355X run is profiles/graph_memset_probe.txt: every buffer is zero after
the first replay, and five of the six hold other bytes after every later one.  That is why the library zeroes with
a kernel (zero_async, csrc/dpr_tiled.h) and refuses rocPRIM's onesweep sort on a capturing stream (csrc/dpr_sort.hip).

    python tools/graph_memset_probe.py
"""
import ctypes

import numpy as np
import torch

hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
hip.hipMemsetAsync.restype = ctypes.c_int


def main():
    dev = torch.device("cuda:0")
    nan = float("nan")
    bufs = {n: torch.full((n,), nan, device=dev) for n in (27, 9, 3, 6, 8, 9003)}
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for t in bufs.values():
            rc = hip.hipMemsetAsync(t.data_ptr(), 0, t.numel() * 4, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
        keep = torch.ones(4, device=dev) * 2  # (a kernel node as well)  # noqa: F841
    rng = np.random.default_rng(0)
    for replay in range(4):
        if replay >= 2:
            for _ in range(7):
                x = torch.as_tensor(rng.random((3001, 3)).astype(np.float32), device=dev)
                torch.empty_like(x).copy_(x)
        for t in bufs.values():
            t.fill_(nan)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        print(f"replay {replay}:", {n: (int((t != 0).sum()),
                                        [hex(x & 0xffffffff) for x in t[-4:].view(torch.int32).tolist()])
                                    for n, t in bufs.items()}, flush=True)


if __name__ == "__main__":
    main()
