// mobi_encode_inter_code.h -- DEVICE ONLY, NO INCLUDE GUARD: the body of the inter encoder's code kernel, included once into each of
// mobi_encode_inter.hip's two kernels, behind `constexpr bool PINTRA`: false in mobi_encp_code, true in mobi_encp_code_pintra, the intra
// mode's (mobi_encode_pintra.h), whose lane 0 leaves the macroblock's cost Jp and its kind word in place of predictor, syntax bits and
// statistics; those wait for the decisions (mobi_encpi_finish, mobi_encode_pintra.hip).  The coding itself is the same text.
// Why text and not a function template: with the body in an inlined function, by reference or by value, the compiler gives mobi_encp_code
// 74 registers where it has 72 as a kernel body, and six waves per SIMD where it has seven; mode 0 must stay the kernel it was.
// A: the kernel's MobiEncInterArgs.
  __shared__ uint32_t lut32[MOBI_TC_LUT_BYTES / 4];
  __shared__ CodeLds lds[WAVES];
  const MobiEncInterConst *K = A.kp;
  const uint8_t *lut = mobi_lanes_stage_lut<WAVES * 64>(K, lut32);
  __syncthreads();
  const int wave = threadIdx.x >> 6, pic = blockIdx.y, nmb = A.mbw * A.mbh, mb = blockIdx.x * WAVES + wave;
  if (mb >= nmb) return; // a whole wave: nothing below synchronises beyond the wave
  CodeLds &L = lds[wave];
  const MobiSyncWave wave_sync;
  const int lane = threadIdx.x & 63, g = lane >> 3, r = lane & 7, k = g < 6 ? g : 0;
  const int mby = mb / A.mbw, mbx = mb - mby * A.mbw, W = A.W, q = A.q[pic];
  const size_t ysz = (size_t)W * A.H, frame = ysz + ysz / 2;
  const uint32_t *mvs = A.mv + (size_t)pic * nmb;
  const uint32_t v = mvs[mb];
  const MobiEncpBlockRef at = mobi_encp_block_ref(k, mbx, mby, W, mobi_encp_dx(v), mobi_encp_dy(v));
  const size_t plane = at.plane ? ysz + (size_t)(at.plane - 1) * (ysz / 4) : 0;
  int zi[8], s[8], p[8], x[8], d[8];
  mobi_lanes_scan<8>(K, r, zi);
  Row<8>::unpack(*(const uint2 *)(A.src + (size_t)pic * A.src_pitch + plane + (size_t)(at.y0 + r) * at.pitch + at.x0), s);
  {
    // the row of the prediction: bytes rx .. rx + 7 (+ 1 for a horizontal phase) of row ry + r (and the row below for a vertical phase),
    // inside the plane's rectangle by mobi_encp_vector_ok; fetched as the aligned words that hold them, the third only when it does
    const int off = at.rx & 3;
    const uint8_t *row = A.ref + (size_t)pic * A.ref_pitch + plane + (size_t)(at.ry + r) * at.pitch + (at.rx - off);
    const bool third = off + (at.phase & 1) > 0;
    const uint32_t *w = (const uint32_t *)row, *wn = (const uint32_t *)(row + at.pitch);
    const uint64_t lo = (uint64_t)w[1] << 32 | w[0];
    const uint32_t hi = third ? w[2] : 0u;
    uint64_t lo2 = 0;
    uint32_t hi2 = 0;
    if (at.phase & 2) {
      lo2 = (uint64_t)wn[1] << 32 | wn[0];
      hi2 = third ? wn[2] : 0u;
    }
    const uint64_t a = bytes8(lo, hi, off), b = bytes8(lo, hi, off + 1), c = bytes8(lo2, hi2, off), e = bytes8(lo2, hi2, off + 1);
    const uint2 pr = {mobi_mc4((uint32_t)a, (uint32_t)b, (uint32_t)c, (uint32_t)e, at.phase),
                      mobi_mc4((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32), (uint32_t)(e >> 32), at.phase)};
    Row<8>::unpack(pr, p);
  }
  // the block coder's steps at wave scope; every group runs them, 6 and 7 too: the shuffles stay convergent
#pragma unroll
  for (int j = 0; j < 8; j++) x[j] = s[j] - p[j];
  mobi_lanes_forward<8>(x, r, L.tile[g], wave_sync, d);
  MobiLaneCoded<8> c;
  mobi_lanes_code<8>(K, lut, q, r, zi, s, p, d, L.tile[g], L.nat[g], wave_sync, c);
  const uint32_t sum2 = mobi_lanes_sum<8>(c.sad_pred | c.range << 14);
  const MobiEncBlock b = mobi_enc_block_result(c.mask != 0, c.clamp(), (sum2 >> 14) != 0, (int)c.bits(), (int)c.sad(), (int)(sum2 & 0x3FFF));
  MobiEncMb *rec_mb = A.mbs + (size_t)pic * nmb + mb;
  if (g < 6) {
    int px[8], lv[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      px[j] = b.coded ? c.px[j] : p[j];
      lv[j] = b.coded ? c.lv[j] : 0;
    }
    *(uint2 *)(A.rec + (size_t)pic * frame + plane + (size_t)(at.y0 + r) * at.pitch + at.x0) = Row<8>::pack(px);
    const int4 l4 = Row<8>::pack_lev(lv);
    uint2 *dst = (uint2 *)(rec_mb->lev[g] + r * 8); // records are 8-byte aligned, not 16
    dst[0] = uint2{(uint32_t)l4.x, (uint32_t)l4.y};
    dst[1] = uint2{(uint32_t)l4.z, (uint32_t)l4.w};
  }
  // every block's figures to every lane: coded, clamp, range, bits (< 2^11), sad (< 2^14)
  const uint32_t mine = (uint32_t)b.coded | (uint32_t)b.clamp << 1 | (uint32_t)b.range << 2 | (uint32_t)b.bits << 3 | (uint32_t)b.sad << 14;
  uint32_t cbp = 0, bits = 0, sad = 0, clamp = 0, range = 0;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    const uint32_t o = (uint32_t)__shfl((int)mine, a * 8);
    cbp |= (o & 1) << a;
    clamp += (o >> 1) & 1;
    range += (o >> 2) & 1;
    bits += (o >> 3) & 0x7FF;
    sad += o >> 14;
  }
  if constexpr (PINTRA) {
    if (lane == 0) {
      rec_mb->bits = bits; // the blocks' alone: the finish pass adds the syntax in front of them
      rec_mb->luma_mode = rec_mb->chroma_mode = rec_mb->pad = 0;
      rec_mb->cbp = (uint8_t)cbp;
      A.jp[(size_t)pic * nmb + mb] = mobi_encpi_jp(K, A.ver, mobi_enc_lambda(q), sad, bits, v, cbp);
      A.kind[(size_t)pic * nmb + mb] = mobi_encpi_kind(false, sad, clamp, range);
    }
    return;
  }
  if (lane == 0) {
    const uint32_t pred = mobi_encp_predictor(mvs, A.mbw, mbx, mby), vb = mobi_encp_mv_bits(K, A.ver, v, pred);
    A.mvp[(size_t)pic * nmb + mb] = pred;
    rec_mb->bits = vb + mobi_encp_cbp_bits(K, cbp) + bits;
    rec_mb->luma_mode = rec_mb->chroma_mode = rec_mb->pad = 0;
    rec_mb->cbp = (uint8_t)cbp;
    if (A.pstats) {
      mobi_enc_inter_stats *st = A.pstats + pic;
      atomicAdd((unsigned long long *)&st->sad, (unsigned long long)sad);
      atomicAdd((unsigned long long *)&st->mv_bits, (unsigned long long)vb);
      if (cbp) atomicAdd(&st->coded_blocks, (uint32_t)__popc(cbp));
      if (clamp) atomicAdd(&st->fallback_clamp, clamp);
      if (range) atomicAdd(&st->fallback_level, range);
      if (v == pred) atomicAdd(&st->code0, 1u);
      if (v) atomicAdd(&st->nonzero_mv, 1u);
      if ((mobi_encp_dx(v) | mobi_encp_dy(v)) & 1) atomicAdd(&st->halfpel_mv, 1u);
    }
  }
