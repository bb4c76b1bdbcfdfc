"""Inside ONE k_fm_update launch of the steady loop: s_memrealtime stamps (100 MHz) of every tile wave -- start, list arrived, loads arrived,
row updates issued, (closing tiles) crossing run done -- for the whole grid and BY POPULATION: tiles of fields of <= 4,096 rows against
tiles of larger fields, closing tiles against the others, under fmx_set_option("upd_order", 0) (index order) and 1 (ascending row count)
in one session.  Which population ends the launch, before and after.  Needs the diagnostic build: tools/update_stamps.sh builds it
with -DFMX_STAMPS."""
import ctypes as C, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fm-for-online-recommendation_amd")); sys.path.insert(0, ROOT)
import fmx, bench
lib = fmx._lib.load()
dev = torch.device("cuda", 0)
sizes = bench.CRITEO_SIZES
F, TPF = len(sizes), 64                      # 4,096 samples: 64 tiles per field; stamps are stored by (field, tile), whatever the dispatch order
SMALL_ROWS = 4096
hyper = fmx.Hyper(**bench.HYPER)
idx_np, y_np = bench.synth_pool(16, 4096, sizes, 1)
idx_pool, y_pool = torch.from_numpy(idx_np).to(dev), torch.from_numpy(y_np).to(dev)
POINTS = ("wave start", "list arrived", "loads arrived", "row updates issued", "closing tile done")


def q(a):
    return "p50 %5.2f  p90 %5.2f  max %5.2f" % tuple(np.percentile(a, [50, 90, 100])) if len(a) else "-"


def session(order):
    table = fmx.FlatTable(sizes, 16, layout="ftrl", device=dev, ftrl=bench.HYPER)
    w0 = torch.randn((table.n_rows, 16), device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 0.01
    table.rows[:, :16] = w0
    table.rows[:, table.z_offset:table.z_offset + 16] = fmx.table.ftrl_z_for_weight_torch(w0, table.ftrl)
    eng = fmx.FMEngine(table, max_batch=4096)
    loss = torch.zeros(2048, device=dev)
    work = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    run = eng.prepare_stream(hyper, "ftrl", "logits", idx_pool, y_pool, loss, stream=work)
    tiles = F * TPF
    small = np.repeat(np.asarray(sizes) <= SMALL_ROWS, TPF)
    ends = []
    for n_steps in (600, 603, 605):          # the last launch of each run: different positions inside a sort group
        run(n_steps)
        torch.cuda.synchronize()
        buf = (C.c_ulonglong * (8192 * 6))()
        assert lib.fmx_debug_update_stamps(buf) == 0
        st = np.frombuffer(buf, dtype=np.uint64).reshape(8192, 6)[:tiles].astype(np.float64) / 100.0      # us
        rel = st - st[:, 0].min()
        closing = st[:, 4] > st[:, 0]
        done = np.where(closing, rel[:, 4], rel[:, 3])        # the wave's last stamp
        print(f"--- upd_order {order}: last update of a {n_steps}-step run ({tiles} tile waves; us from the first wave's start) ---")
        pops = (("all tiles", np.ones(tiles, bool)), (f"fields <= {SMALL_ROWS} rows", small), (f"fields > {SMALL_ROWS} rows", ~small),
                ("closing tiles", closing), ("other tiles", ~closing), ("small, closing", small & closing), ("large, closing", ~small & closing))
        for name, m in pops:
            print(f"  {name} ({int(m.sum())} tiles)")
            for s, point in enumerate(POINTS):
                mm = m & closing if s == 4 else m
                if mm.any():
                    print(f"    {point:<20s}{q(rel[mm, s])}")
            print(f"    {'last stamp':<20s}{q(done[m])}")
        last = int(done.argmax())
        print(f"  the launch ends with field {last // TPF} ({sizes[last // TPF]} rows), tile {last % TPF}, "
              f"{'closing' if closing[last] else 'ordinary'}, at {done[last]:.2f} us; hand-off of the closing tiles p50 "
              f"{np.median(rel[closing, 4] - rel[closing, 3]) if closing.any() else 0.0:.2f} us")
        ends.append(done.max())
    return ends


res = {}
for order in (0, 1):
    prev = lib.fmx_set_option(b"upd_order", order)
    try:
        res[order] = session(order)
    finally:
        lib.fmx_set_option(b"upd_order", prev)
print("last stamp of the launch, us:", {k: [round(x, 2) for x in v] for k, v in res.items()})
