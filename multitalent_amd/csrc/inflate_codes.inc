// inflate_codes.inc — included inside the block loop of a decoding wave (inflate.hip, inflate_spec.hip), behind the block's three
// header bits: reads the two codes of a fixed (type 1) or dynamic (type 2) block from `I` and builds their tables in `T`.  Uses
// the wave's `lane`, `type` and `status`; an invalid header, an over-subscribed code or a read behind the input sets IF_BAD and
// leaves the block loop.
    // ---- the two codes
    int hlit = 288, hdist = 30;
    if (type == 1) {
      __syncthreads();
      for (int s = lane; s < 320; s += IF_WAVE) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    } else {
      hlit = (int)I.get(5) + 257;
      hdist = (int)I.get(5) + 1;
      const int hclen = (int)I.get(4) + 4;
      if (hlit > 286 || hdist > 30) { status = IF_BAD; break; }
      __syncthreads();
      if (lane < 19) T.lens[lane] = 0;
      __syncthreads();
      for (int k = 0; k < hclen; ++k) { const uint32_t v = I.get(3); if (lane == 0) T.lens[IF_ORDER[k]] = (uint8_t)v; }
      if (I.overrun() || !if_build(T, T.lens, 19, T.cntc, T.symc, nullptr, 0, lane)) { status = IF_BAD; break; }
      int i = 0, prev = 0;
      const int total = hlit + hdist;
      while (i < total) {
        I.refill();
        int len;
        const int s = __builtin_amdgcn_readfirstlane(if_walk(T.cntc, T.symc, I.bb, 7, len));
        len = __builtin_amdgcn_readfirstlane(len);
        if (s < 0) { status = IF_BAD; break; }
        I.take(len);
        if (s < 16) {
          if (lane == 0) T.lens[i] = (uint8_t)s;
          ++i; prev = s;
        } else {
          int rep, val = 0;
          if (s == 16) { if (i == 0) { status = IF_BAD; break; } val = prev; rep = 3 + (int)I.get(2); }
          else if (s == 17) rep = 3 + (int)I.get(3);
          else rep = 11 + (int)I.get(7);
          if (i + rep > total) { status = IF_BAD; break; }
          for (int k = lane; k < rep; k += IF_WAVE) T.lens[i + k] = (uint8_t)val;
          i += rep; prev = val;
        }
        if (I.overrun()) { status = IF_BAD; break; }
      }
      if (status != IF_OK) break;
      __syncthreads();
      if (T.lens[256] == 0) { status = IF_BAD; break; }
    }
    const bool okl = if_build(T, T.lens, hlit, T.cntl, T.syml, T.fastl, IF_FASTL, lane);
    const bool okd = if_build(T, T.lens + hlit, hdist, T.cntd, T.symd, T.fastd, IF_FASTD, lane);
    if (!okl || !okd) { status = IF_BAD; break; }
