// fmx_rank_host.inc -- the entry points of the rank calls (include/fmx.h), included at the end of fmx_topk.hip

namespace {

// the bounds on U * splits of the three top-K workspaces, monotone in U and N
inline int64_t fm_rank_parts(int U, int N) {
  const int64_t sn = std::min<int64_t>(TK_MAX_SPLITS, (N + TK_SPLIT_MIN - 1) / TK_SPLIT_MIN);
  return std::min<int64_t>((int64_t)U * sn, (int64_t)U + (int64_t)TK_TILE_BUDGET * TK_MAX_UT);
}
inline int64_t mlp_rank_parts(const MlpShape &s, int U, int N) {
  return std::min<int64_t>((int64_t)U * tm_max_splits(s, N), (int64_t)U + TM_TILE_BUDGET);
}
inline int64_t afm_rank_parts(const fmx_afm_t *afm, int n_ctx, int n_item, int U, int N) {
  const int64_t sm = at_split_min(n_ctx, n_item, afm->t, at_kp(afm->k));
  return std::min<int64_t>((int64_t)U * at_max_splits(sm, N), (int64_t)U + AT_TILE_BUDGET);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int check_rank_sizes(const char *fn, int32_t U, int32_t N, int32_t T) {
  if (U < 1 || N < 1) return fail(FMX_ERR_ARG, "%s: U=%d and N=%d must be >= 1", fn, U, N);
  if (T < 1) return fail(FMX_ERR_ARG, "%s: T=%d must be >= 1", fn, T);
  if (T > RK_MAX_T) return fail(FMX_ERR_UNSUPPORTED, "%s: T=%d, one call covers T <= %d targets per user", fn, T, RK_MAX_T);
  return FMX_OK;
}
int check_rank_flag(const char *fn, int32_t filtered) {
  if (filtered != 0 && filtered != 1) return fail(FMX_ERR_ARG, "%s: filtered=%d must be 0 or 1", fn, filtered);
  return FMX_OK;
}
int check_rank_ws(const char *fn, int64_t ws_bytes, int64_t need) {
  if (ws_bytes < need)
    return fail(FMX_ERR_SHAPE, "%s: workspace of %lld bytes, %s_workspace_bytes = %lld", fn, (long long)ws_bytes, fn, (long long)need);
  return FMX_OK;
}

// the keys and the partial counts at `base` of the workspace
inline RankIo rank_io(void *base, const int32_t *targets, int U, int T) {
  char *b = static_cast<char *>(base);
  return RankIo{targets, reinterpret_cast<uint64_t *>(b), reinterpret_cast<int32_t *>(b + rank_keys_bytes(U, T)), T};
}

}  // namespace

extern "C" {

int64_t fmx_fm_rank_workspace_bytes(int32_t U, int32_t N, int32_t T) {
  if (int rc = check_rank_sizes("fmx_fm_rank", U, N, T)) return rc;
  return rank_ws_bytes(fm_rank_parts(U, N), U, T);
}

int fmx_fm_rank(const float *Su, int32_t ld_u, const float *au, int32_t U, const float *Sc, int32_t ld_c, const float *ac, int32_t N,
                int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos, const int32_t *targets, int32_t T, int32_t filtered,
                void *workspace, int64_t workspace_bytes, int32_t *rank_out, float *score_out, int32_t *n_cand_out,
                fmx_stream_t stream) {
  const char *fn = "fmx_fm_rank";
  if (int rc = check_pair_ptrs(fn, Su, au, Sc, ac, excl_offsets, excl_pos, workspace, targets, rank_out)) return rc;
  if (int rc = check_rank_sizes(fn, U, N, T)) return rc;
  if (int rc = check_rank_flag(fn, filtered)) return rc;
  if (int rc = check_pair_layout(fn, FMX_ERR_SHAPE, Su, ld_u, Sc, ld_c, kp, workspace)) return rc;
  if (int rc = check_rank_ws(fn, workspace_bytes, rank_ws_bytes(fm_rank_parts(U, N), U, T))) return rc;
  const TopkGeom g = topk_geom(U, N, 1);
  FmRankArgs a{TopkArgs{Su, au, Sc, ac, excl_offsets, excl_pos, nullptr, nullptr, nullptr, ld_u, ld_c, U, N, 1, g.ut, g.cap, g.splits, g.per},
               rank_io(workspace, targets, U, T)};
  FmRankArgs ka = a;  // phase 1: one user per workgroup
  ka.ut = 1;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 kgrid(U, T), grid(g.tiles, g.splits), block(TK_THREADS);
  int rc;
#define FMX_FM_RANK(KP)                                                                       \
  hipLaunchKernelGGL((k_topk_scan<KP, SCAN_KEYS, FmRankArgs>), kgrid, block, 0, st, ka);      \
  if ((rc = check_launch("k_topk_scan (rank keys)"))) return rc;                              \
  hipLaunchKernelGGL((k_topk_scan<KP, SCAN_COUNT, FmRankArgs>), grid, block, 0, st, a);       \
  rc = check_launch("k_topk_scan (rank count)")
  switch (kp) {
    case 4: FMX_FM_RANK(4); break;
    case 8: FMX_FM_RANK(8); break;
    case 16: FMX_FM_RANK(16); break;
    case 32: FMX_FM_RANK(32); break;
    default: FMX_FM_RANK(64); break;
  }
#undef FMX_FM_RANK
  if (rc) return rc;
  return finish_rank(a.r, excl_offsets, excl_pos, U, N, g.splits, filtered, rank_out, score_out, n_cand_out, st);
}

int64_t fmx_mlp_rank_workspace_bytes(const fmx_mlp_t *mlp, int32_t U, int32_t N, int32_t T) {
  if (!mlp) return fail(FMX_ERR_ARG, "fmx_mlp_rank: null mlp");
  if (int rc = check_rank_sizes("fmx_mlp_rank", U, N, T)) return rc;
  if (int rc = check_network(mlp, "fmx_mlp_rank")) return rc;
  const MlpShape sh = mlp_shape(mlp);
  return mlp_packed_floats(sh, nullptr) * 4 + rank_ws_bytes(mlp_rank_parts(sh, U, N), U, T);
}

int fmx_mlp_rank(const fmx_mlp_t *mlp, int32_t fm_term, const float *Su, const float *Bu, int32_t ld_u, const float *au, int32_t U,
                 const float *Sc, const float *Bc, int32_t ld_c, const float *ac, int32_t N, int32_t kp, const int32_t *excl_offsets,
                 const int32_t *excl_pos, const int32_t *targets, int32_t T, int32_t filtered, void *workspace, int64_t workspace_bytes,
                 int32_t *rank_out, float *score_out, int32_t *n_cand_out, fmx_stream_t stream) {
  const char *fn = "fmx_mlp_rank";
  if (!mlp || !mlp->params || !Bu || !Bc) return fail(FMX_ERR_ARG, "%s: null argument", fn);
  if (fm_term != 0 && fm_term != 1) return fail(FMX_ERR_ARG, "%s: fm_term=%d must be 0 or 1", fn, fm_term);
  if (int rc = check_network(mlp, fn)) return rc;
  if (mlp->k > kp) return fail(FMX_ERR_UNSUPPORTED, "%s: k=%d exceeds kp=%d", fn, mlp->k, kp);
  const MlpShape sh = mlp_shape(mlp);
  if (int rc = check_pair_ptrs(fn, Su, au, Sc, ac, excl_offsets, excl_pos, workspace, targets, rank_out)) return rc;
  if (int rc = check_rank_sizes(fn, U, N, T)) return rc;
  if (int rc = check_rank_flag(fn, filtered)) return rc;
  if (int rc = check_pair_layout(fn, FMX_ERR_UNSUPPORTED, Su, ld_u, Sc, ld_c, kp, workspace)) return rc;
  const int64_t packed_bytes = mlp_packed_floats(sh, nullptr) * 4;
  if (int rc = check_rank_ws(fn, workspace_bytes, packed_bytes + rank_ws_bytes(mlp_rank_parts(sh, U, N), U, T))) return rc;
  if (!aligned16(Bu) || !aligned16(Bc)) return fail(FMX_ERR_ALIGN, "%s: Bu and Bc must be 16-byte aligned", fn);
  const MlpTopkGeom g = mlp_topk_geom(sh, U, N, 1);
  MlpPackArgs p{mlp->params, static_cast<float *>(workspace), {}, {}, {}, {}, 0, sh.k, sh.H, sh.L, sh.K0, sh.Hp, sh.NT};
  p.total = mlp_packed_floats(sh, &p);
  MlpRankArgs a{MlpTopkArgs{Su, Bu, au, Sc, Bc, ac, excl_offsets, excl_pos, p.packed, {}, {}, nullptr, nullptr, nullptr,
                            ld_u, ld_c, U, N, 1, kp, sh.k, sh.H, sh.L, sh.K0, sh.Hp, fm_term, g.cap, g.splits, g.per},
                rank_io(static_cast<char *>(workspace) + packed_bytes, targets, U, T)};
  std::copy(p.dst_w, p.dst_w + sh.L, a.woff);
  std::copy(p.dst_b, p.dst_b + sh.L, a.boff);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_mlp_topk_pack, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, st, p);
  if (int rc = check_launch("k_mlp_topk_pack")) return rc;
  const dim3 kgrid(U, T), grid(U, g.splits);
  const size_t lds = (size_t)TM_ROWS * std::max(sh.K0, sh.Hp) * 4;  // the activations; the counters are static LDS
  int rc;
#define FMX_MLP_RANK(WC, NCT)                                                                                                \
  rc = launch_slots<k_mlp_topk_scan<WC, NCT, SCAN_KEYS, MlpRankArgs>>("k_mlp_topk_scan (rank keys)", kgrid, lds, st, a);     \
  if (!rc) rc = launch_slots<k_mlp_topk_scan<WC, NCT, SCAN_COUNT, MlpRankArgs>>("k_mlp_topk_scan (rank count)", grid, lds, st, a)
  switch (sh.NT) {  // the wave grids of fmx_mlp_topk
    case 1: FMX_MLP_RANK(1, 1); break;
    case 2: FMX_MLP_RANK(2, 1); break;
    case 3: FMX_MLP_RANK(2, 2); break;
    case 4: FMX_MLP_RANK(4, 1); break;
    case 5: case 6: case 7: case 8: FMX_MLP_RANK(4, 2); break;
    case 9: case 10: case 11: case 12: FMX_MLP_RANK(4, 3); break;
    default: FMX_MLP_RANK(4, 4); break;
  }
#undef FMX_MLP_RANK
  if (rc) return rc;
  return finish_rank(a.r, excl_offsets, excl_pos, U, N, g.splits, filtered, rank_out, score_out, n_cand_out, st);
}

int64_t fmx_afm_rank_workspace_bytes(const fmx_afm_t *afm, int32_t n_ctx, int32_t n_item, int32_t U, int32_t N, int32_t T) {
  if (!afm) return fail(FMX_ERR_ARG, "fmx_afm_rank: null afm");
  if (int rc = check_rank_sizes("fmx_afm_rank", U, N, T)) return rc;
  if (int rc = check_afm_pair_shape("fmx_afm_rank", afm, n_ctx, n_item)) return rc;
  return at_packed_bytes(afm->t) + rank_ws_bytes(afm_rank_parts(afm, n_ctx, n_item, U, N), U, T);
}

int fmx_afm_rank(const fmx_afm_t *afm, const float *Eu, const float *stats_u, int32_t n_ctx, int32_t U, const float *Ec,
                 const float *stats_c, int32_t n_item, int32_t N, int32_t kp, const int32_t *excl_offsets, const int32_t *excl_pos,
                 const int32_t *targets, int32_t T, int32_t filtered, void *workspace, int64_t workspace_bytes, int32_t *rank_out,
                 float *score_out, int32_t *n_cand_out, fmx_stream_t stream) {
  const char *fn = "fmx_afm_rank";
  if (!afm) return fail(FMX_ERR_ARG, "%s: null afm", fn);
  if (int rc = check_rank_sizes(fn, U, N, T)) return rc;
  if (int rc = check_afm_pair_shape(fn, afm, n_ctx, n_item)) return rc;
  if (int rc = check_afm_pair_args(fn, afm, Eu, stats_u, Ec, stats_c, kp, excl_offsets, excl_pos, workspace, targets, rank_out)) return rc;
  if (int rc = check_rank_flag(fn, filtered)) return rc;
  const int64_t need = at_packed_bytes(afm->t) + rank_ws_bytes(afm_rank_parts(afm, n_ctx, n_item, U, N), U, T);
  if (int rc = check_rank_ws(fn, workspace_bytes, need)) return rc;
  const AfmGeom g = afm_scan_geom(afm, n_ctx, n_item, U, N);
  AfmRankArgs a{AfmTopkArgs{Eu, stats_u, Ec, stats_c, static_cast<const float *>(workspace), excl_offsets, excl_pos, nullptr, nullptr,
                            nullptr, U, N, 1, afm->t, n_ctx, n_item, topk_cap(1), g.splits, g.per},
                rank_io(static_cast<char *>(workspace) + at_packed_bytes(afm->t), targets, U, T)};
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int packed_n = afm->t * kp + 2 * afm->t + kp;
  hipLaunchKernelGGL(k_afm_topk_pack, dim3((packed_n + 255) / 256), dim3(256), 0, st, afm->params, afm->k, afm->t, kp,
                     static_cast<float *>(workspace));
  if (int rc = check_launch("k_afm_topk_pack")) return rc;
  const dim3 kgrid(U, T), grid(U, g.splits), block(TK_THREADS);
  int rc;
#define FMX_AFM_RANK(KP)                                                                          \
  hipLaunchKernelGGL((k_afm_topk_scan<KP, SCAN_KEYS, AfmRankArgs>), kgrid, block, 0, st, a);      \
  if ((rc = check_launch("k_afm_topk_scan (rank keys)"))) return rc;                              \
  hipLaunchKernelGGL((k_afm_topk_scan<KP, SCAN_COUNT, AfmRankArgs>), grid, block, 0, st, a);      \
  rc = check_launch("k_afm_topk_scan (rank count)")
  switch (kp) {
    case 4: FMX_AFM_RANK(4); break;
    case 8: FMX_AFM_RANK(8); break;
    case 16: FMX_AFM_RANK(16); break;
    case 32: FMX_AFM_RANK(32); break;
    default: FMX_AFM_RANK(64); break;
  }
#undef FMX_AFM_RANK
  if (rc) return rc;
  return finish_rank(a.r, excl_offsets, excl_pos, U, N, g.splits, filtered, rank_out, score_out, n_cand_out, st);
}

}  // extern "C"
