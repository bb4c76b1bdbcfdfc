"""Inside ONE k_fm_forward launch of the steady loop (bench.py's FM + FTRL step, B = 4096): s_memrealtime stamps (100 MHz) of every
wave -- start, indices / offsets / label arrived, rows arrived, butterfly done, epilogue done, stores issued.  Needs the diagnostic
build (tools/forward_stamps.sh build, -DFMX_STAMPS); FMX_LIB_PATH names another diagnostic build of the same ABI."""
import ctypes as C, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd")); sys.path.insert(0, ROOT)
import fmx, bench
lib = fmx._lib.load()
dev = torch.device("cuda", 0)
sizes, B = bench.CRITEO_SIZES, bench.BATCH
hyper = fmx.Hyper(**bench.HYPER)
table = fmx.FlatTable(sizes, 16, layout="ftrl", device=dev, ftrl=bench.HYPER)
w0 = torch.randn((table.n_rows, 16), device=dev) * 0.01
table.rows[:, :16] = w0
table.rows[:, table.z_offset:table.z_offset + 16] = fmx.table.ftrl_z_for_weight_torch(w0, table.ftrl)
eng = fmx.FMEngine(table, max_batch=B)
idx_np, y_np = bench.synth_pool(16, B, sizes, 1)
idx_pool, y_pool = torch.from_numpy(idx_np).to(dev), torch.from_numpy(y_np).to(dev)
loss = torch.zeros(2048, device=dev)
work = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
run = eng.prepare_stream(hyper, "ftrl", "logits", idx_pool, y_pool, loss, stream=work)
names = ["wave start", "indices arrived", "rows arrived", "butterfly done", "epilogue done", "stores issued"]
print(f"library: {fmx._lib.LIB_PATH}")
for n_steps in (600, 603, 605):          # the last launch of each run: different positions inside a sort group
    run(n_steps)
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * (8192 * 6))()
    assert lib.fmx_debug_forward_stamps(buf) == 0
    st = np.frombuffer(buf, dtype=np.uint64).reshape(8192, 6)[:B].astype(np.float64) / 100.0      # us
    rel = st - st[:, 0].min()
    def q(a): return "p10 %5.2f  p50 %5.2f  p90 %5.2f  max %5.2f" % tuple(np.percentile(a, [10, 50, 90, 100]))
    print(f"--- last forward of a {n_steps}-step run ({B} waves; us from the first wave's start) ---")
    for i, nm in enumerate(names):
        print(f"{nm:<18}", q(rel[:, i]))
    print("per wave, from the previous point:")
    for i in range(1, 6):
        print(f"  {names[i - 1]:>16} -> {names[i]:<16}", q(rel[:, i] - rel[:, i - 1]))
    print(f"  {'wave start':>16} -> {'stores issued':<16}", q(rel[:, 5] - rel[:, 0]))
    print("first wave start -> last store issued  %.2f us;  last wave start %.2f us" % (rel[:, 5].max(), rel[:, 0].max()))
