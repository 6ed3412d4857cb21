// mobi_mux_append_body.h -- the body of mobi_mux_append and mobi_mux_append_audio (mobi_mux.hip), included into each with
// MUX_STREAM_INDEX defined: 0 video, 1 audio.  No include guard: it is text, not declarations.
  const int clip = blockIdx.y;
  const int32_t size = A.sizes[clip];
  const MobiMuxState s = A.state[clip];
  if (mobi_mux_frame_status(A.cfg, s, size, A.slot_bytes, A.capacity, A.key_frame)) return;
  const uint32_t pieces = mobi_mux_pieces(A.cfg.container, (uint64_t)size);
  const uint8_t *slot = A.slots + (uint64_t)clip * A.slot_pitch;
  uint8_t *at = A.files + (uint64_t)clip * A.pitch + s.pos;
  const uint32_t lane = threadIdx.x;
  for (uint32_t p = blockIdx.x; p < pieces; p += gridDim.x) {
    const MobiMuxPiece q = mobi_mux_piece(A.cfg.container, (uint64_t)size, p, MUX_STREAM_INDEX);
    uint8_t *d = at + q.dst;
    mux_copy(d + q.head_n, slot + q.src, q.len, lane);
    if (lane >= 32 && lane < 32 + MOBI_MUX_PIECE_HEAD_MAX) {
      const uint32_t i = lane - 32;
      if (i < q.head_n) d[i] = mobi_mux_piece_head(q, i);
    } else if (lane == 32 + MOBI_MUX_PIECE_HEAD_MAX && q.term) {
      d[q.head_n + q.len] = 0;
    }
  }
