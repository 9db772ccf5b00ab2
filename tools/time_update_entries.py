"""Host cost of one small update call: ht_update_dev on one 64x64 tile, and ht_update_hands_dev with flags on four.
    python tools/time_update_entries.py [calls]      (HT_LIB_PATH=<another build> for an A/B on one device)
Per call: `enqueue` is the host time inside the call (nothing is waited for), `done` the time until the stream has drained.  Prints one JSON line with the medians in us."""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hand_tracking_samples_amd import native, weights as W
N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
d = np.load(os.path.join(ROOT, "bench_data", "frames1024.npz"))
dev = torch.device("cuda:0")
c = native.Context(os.path.join(ROOT, "hand_tracking_samples_amd", "assets", "model_hand17.htfx"), 4)
c.load_weights(W.make_cnnb()); c.set_params(microforce=3.0, mainthreadpasses=3)
depth = torch.from_numpy(np.ascontiguousarray(d["depth"][:4]).reshape(4, -1).view(np.int16)).to(dev); cams = torch.from_numpy(d["cam"][:4]).to(dev); start = torch.from_numpy(d["startpose"][:4]).to(dev)
hands = torch.tensor([0, 1, 1, 0], dtype=torch.uint8, device=dev); out = torch.empty((4, 17, 7), dtype=torch.float32, device=dev)
s = torch.cuda.current_stream(dev)
p = [t.data_ptr() for t in (depth, cams, start, out, hands)]
calls = {"update_dev B=1 tile": lambda: c.update_dev(p[0], p[1], p[2], 1, p[3], s.cuda_stream),
         "update_hands_dev B=4 flags": lambda: c.update_hands_dev(64, p[0], p[1], 64, 64, 0.17, p[4], p[2], 4, p[3], s.cuda_stream)}
res = {"lib": os.path.basename(os.path.dirname(native.lib_path())), "calls": N}
for name, call in calls.items():
    enq, done = [], []
    for i in range(N + 20):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); call(); t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
        if i >= 20:
            enq.append(t1 - t0); done.append(t2 - t0)
    res[name] = {"enqueue_us": round(float(np.median(enq)) * 1e6, 2), "done_us": round(float(np.median(done)) * 1e6, 2)}
c.close()
print(json.dumps(res), flush=True)
