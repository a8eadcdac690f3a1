// cg_hmarl_body.inc -- steps 3 to 5 of the H-MARL decode (cg_hmarl.hpp), the text hmarl_kernel<OUTS, TRAIN> and hmarl_pop_kernel<OUTS> both
// include.  The including kernel has declared: q (the cygym_hmarl: status), tb (what holds the strategy's tables -- kind, cost_comp,
// cost_not, batch_len, budget, fanout, fallback: the cygym_hmarl itself, or the cygym_hmarl_slot of the wave's slot), dst, M, fl, dstatic,
// keys, ord, lane, row, tick, env_g, k0, k1 and t (the action type, uniform, 0 .. 31).
  // ---------------- 3. the ordered target list ----------------
  int kind = hm_byte(tb.kind, t);
  int n = 0;   // length of the list (uniform)
  if (kind == CG_HMARL_HIGH) {   // _high_value_targets (:139-154): the !NYA devices by descending score, ties in ascending id
    auto cls_of = [&](const int d) -> int {   // 0: score 100 | 1: 50 | 2: 40 | 3: 20 | 4: 0 | -1: not in the list
      if (d >= M) return -1;
      const uint32_t f = fl[d];
      if (f & CG_F_NYA) return -1;
      if (f & CG_F_COMP) return (f & CG_F_OWNED) ? 2 : ((dstatic[d] & CG_D_DC) ? 0 : 1);
      return (f & CG_F_REACH) ? 3 : 4;
    };
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int d0 = 0; d0 < M; d0 += WAVE) {
      const int c = cls_of(d0 + lane);
      c0 += __popcll(__ballot(c == 0)); c1 += __popcll(__ballot(c == 1)); c2 += __popcll(__ballot(c == 2));
      c3 += __popcll(__ballot(c == 3)); c4 += __popcll(__ballot(c == 4));
    }
    int b0 = 0, b1 = c0, b2 = b1 + c1, b3 = b2 + c2, b4 = b3 + c3;   // class bases, then running
    n = b4 + c4;
    for (int d0 = 0; d0 < M; d0 += WAVE) {
      const int d = d0 + lane, c = cls_of(d);
      const uint64_t m0 = __ballot(c == 0), m1 = __ballot(c == 1), m2 = __ballot(c == 2), m3 = __ballot(c == 3), m4 = __ballot(c == 4);
      const uint64_t mine = c == 0 ? m0 : c == 1 ? m1 : c == 2 ? m2 : c == 3 ? m3 : m4;
      const int base = c == 0 ? b0 : c == 1 ? b1 : c == 2 ? b2 : c == 3 ? b3 : b4;
      if (c >= 0) ord[base + below(mine)] = (uint16_t)(d | (c <= 2 ? 0x8000 : 0));   // (base + prefix < n <= M)
      b0 += __popcll(m0); b1 += __popcll(m1); b2 += __popcll(m2); b3 += __popcll(m3); b4 += __popcll(m4);
    }
    wsync();
  } else if (kind == CG_HMARL_SHUFFLE) {   // attacker type 1 (:263-267): the seeds, or every !NYA device when there is none, shuffled
    bool any = false;
    for (int d0 = 0; d0 < M; d0 += WAVE) {
      const int d = d0 + lane;
      const uint32_t f = d < M ? fl[d] : CG_F_NYA;
      any = any || __ballot(!(f & CG_F_NYA) && (f & (CG_F_OWNED | CG_F_COMP))) != 0ull;
    }
    for (int d0 = 0; d0 < M; d0 += WAVE) {
      const int d = d0 + lane;
      const uint32_t f = d < M ? fl[d] : CG_F_NYA;
      const bool on = !(f & CG_F_NYA) && (!any || (f & (CG_F_OWNED | CG_F_COMP)));
      const uint64_t m = __ballot(on);
      if (on) keys[n + below(m)] = ((uint64_t)cg_philox4x32_10(env_g, tick, CG_SITE_HMARL_SHUFFLE, (uint32_t)d & 0xFFFFu, k0, k1).v[0] << 32) | (uint32_t)d;
      n += __popcll(m);
    }
    wsync();
    for (int i0 = 0; i0 < n; i0 += WAVE) {   // rank = the number of smaller (key, id) pairs; the pairs are distinct
      const int i = i0 + lane;
      const uint64_t mine = i < n ? keys[i] : 0ull;
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += keys[j] < mine ? 1 : 0;   // (uniform address: a broadcast read)
      if (i < n) {
        const int d = (int)(uint32_t)mine;
        ord[rank] = (uint16_t)(d | ((fl[d] & CG_F_COMP) ? 0x8000 : 0));   // (rank < n <= M)
      }
    }
    wsync();
  }
  if (kind >= CG_HMARL_HIGH && n == 0) kind = CG_HMARL_FALLBACK;   // a per-device type whose list is empty (:309-312)
  const int G = dst.max_groups, L = dst.max_devs;
  int16_t* out = const_cast<int16_t*>(dst.dev_idx) + (size_t)row * L;
  const RowGroups og(dst, row);
  if (kind < CG_HMARL_HIGH) {   // (uniform) ONE empty group: [(t, [0], [], 0)], the fallback's type for the fallback (G >= 1)
    if (kind == CG_HMARL_FALLBACK) t = tb.fallback;
    if (lane == 0) {
      og.set(0, t, 0, 1, 0);
      og.dev_cnt[0] = 0;
      const_cast<int32_t*>(dst.n_groups)[row] = 1;
    }
    return;
  }
  // ---------------- 4. + 5. batches (_batch_devices_by_cost, :170-187) and groups (_batchify, :297-308) ----------------
  const double cc = tb.cost_comp[t], cn = tb.cost_not[t], budget = tb.budget;
  const int blen = tb.batch_len[t], fan = tb.fanout;
  double cur = 0.0;      // the sequential walk's running cost
  int inb = 0;           // ... and the devices of its current batch
  int nb = 0;            // batches started before this block of 64 positions
  int last_s = 0;        // position of the last batch start before this block
  int kept = 0;          // list entries written (or cut at L) before this block
  for (int p0 = 0; p0 < n; p0 += WAVE) {
    const int pos = p0 + lane;
    const bool valid = pos < n;
    const uint32_t e = valid ? ord[pos] : 0u;
    uint64_t m;   // batch starts among the block's positions
    if (blen > 0) {
      m = __ballot(valid && pos % blen == 0);
    } else {   // the reference's loop, in its order and in float64; every lane walks alike
      const uint64_t cm = __ballot((e & 0x8000u) != 0u);
      const int nv = n - p0 < WAVE ? n - p0 : WAVE;
      m = p0 == 0 ? 1ull : 0ull;
      for (int j = 0; j < nv; ++j) {
        const double dcost = ((cm >> j) & 1ull) ? cc : cn;
        if (inb > 0 && cur + dcost > budget) { m |= 1ull << j; cur = 0.0; inb = 0; }
        cur += dcost;
        ++inb;
      }
    }
    const uint64_t incl = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull)), excl = m & ((1ull << lane) - 1ull);
    const int my_s = incl ? p0 + hm_top(incl) : last_s;
    const int b = nb + __popcll(incl) - 1;   // (position 0 is a start: b >= 0)
    const bool keep = valid && pos - my_s < fan;   // MAX_FANOUT (:304-306): the batch keeps its first ids and DROPS the rest
    const uint64_t km = __ballot(keep);
    const int opos = kept + below(km);
    if (keep && b < G && opos < L) out[opos] = (int16_t)(e & 0x7FFFu);
    if (valid && ((m >> lane) & 1ull)) {
      if (b < G) og.set(b, t, 0, 1, 0);
      if (b >= 1 && b - 1 < G) {   // the batch that ends here: its count, cut to what is left of the row's L entries
        const int len = pos - (excl ? p0 + hm_top(excl) : last_s);
        int c = len < fan ? len : fan;
        const int ob = opos - c;   // (opos = the entries of all earlier batches)
        c = ob >= L ? 0 : (ob + c > L ? L - ob : c);
        og.dev_cnt[b - 1] = c;
      }
    }
    nb += __popcll(m);
    if (m) last_s = p0 + hm_top(m);
    kept += __popcll(km);
  }
  if (lane == 0) {
    if (nb - 1 < G) {   // the last batch
      const int len = n - last_s;
      int c = len < fan ? len : fan;
      const int ob = kept - c;
      c = ob >= L ? 0 : (ob + c > L ? L - ob : c);
      og.dev_cnt[nb - 1] = c;
    }
    const_cast<int32_t*>(dst.n_groups)[row] = nb < G ? nb : G;
    if (nb > G || kept > L) RowGroups::truncated(q.status);
  }
