// ckm_debug.hip -- diagnostics entries used by the parity tests: every stage of chosen (model, sequence) pairs without filtering,
// envelope rescoring of chosen envelopes, the trace ensemble of a chosen region.
#include "ckm_host.h"

// ---- diagnostics -------------------------------------------------------------------------------------
extern "C" int ckm_debug_stages(ckm_ctx *ctx_, const ckm_profiles *p, const ckm_seqs *s, const uint32_t *model, const uint32_t *seq,
                                uint32_t npairs, ckm_stage_scores *out) {
  return guarded([&] {
    if (!ctx_ || !p || !s || !model || !seq || !out) throw Error(CKM_EINVAL, "NULL argument");
    for (uint32_t j = 0; j < npairs; ++j) if (model[j] < p->hmm.size() && p->too_long[model[j]]) throw Error(CKM_ERANGE, "model longer than the instantiated kernel classes");
    ctx_->settle();
    Worker *ctx = &ctx_->w[0];
    ctx->plan_key.clear();                 // this entry overwrites the worker's SSV tables
    HIPCHK(hipSetDevice(ctx->device));
    const DevModel *dm = p->d_models.as<DevModel>();
    const LenEntry *lt = s->d_lentab.as<LenEntry>();
    const uint8_t *res = s->d_res.as<uint8_t>();
    const uint64_t *off = s->d_off.as<uint64_t>();
    const int32_t *dlen = s->d_len.as<int32_t>();
    memset(out, 0, sizeof(*out) * npairs);
    // SSV: one block per pair (count = 1)
    std::vector<SsvBlockWork> work(npairs); std::vector<uint32_t> ids(seq, seq + npairs);
    std::map<int, std::vector<uint32_t>> byQ;
    for (uint32_t i = 0; i < npairs; ++i) {
      if (model[i] >= p->hmm.size() || seq[i] >= s->nseq) throw Error(CKM_EINVAL, "pair index out of range");
      work[i].model = model[i]; work[i].list_start = i; work[i].count = 1; work[i].pair_start = i; byQ[ssv_class(p->prof[model[i]])].push_back(i);
    }
    std::vector<SsvBlockWork> sorted; std::vector<std::pair<int, std::pair<size_t, size_t>>> groups;
    for (auto &kv : byQ) { groups.push_back({kv.first, {sorted.size(), kv.second.size()}}); for (uint32_t i : kv.second) sorted.push_back(work[i]); }
    ctx->work.ensure(npairs * sizeof(SsvBlockWork)); ctx->idx.ensure(npairs * 4); ctx->maxv.ensure(npairs * 2 + 64);
    wcopy(ctx, ctx->work.p, sorted.data(), npairs * sizeof(SsvBlockWork), hipMemcpyHostToDevice);
    wcopy(ctx, ctx->idx.p, ids.data(), npairs * 4, hipMemcpyHostToDevice);
    SsvEpi epi; memset(&epi, 0, sizeof(epi));
    epi.lentab = lt; epi.maxv = ctx->maxv.as<uint16_t>();              // diagnostics: Smax per pair, no finish
    for (auto &g : groups)
      if (launch_ssv(g.first, (int)g.second.second, ssv_threads_for(g.first), ctx->stream, ctx->work.as<SsvBlockWork>() + g.second.first, dm, res, off, dlen,
                     ctx->idx.as<uint32_t>(), epi))
        throw Error(CKM_ERANGE, "no SSV kernel instance");
    HIPCHK(hipGetLastError());
    std::vector<uint16_t> maxv(npairs);
    HIPCHK(hipMemcpyAsync(maxv.data(), ctx->maxv.p, npairs * 2, hipMemcpyDeviceToHost, ctx->stream));
    // full MSV on every pair: first with the packed kernel the search uses (msv16_kernel, scores only), then with the wave-per-pair kernel
    std::vector<PairRec> pr(npairs);
    for (uint32_t i = 0; i < npairs; ++i) { pr[i].model = model[i]; pr[i].seq = seq[i]; pr[i].usc = 0; pr[i].filtersc = 0; }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::vector<float> uscp; std::vector<int32_t> xJp;
    run_msv_exact(ctx, p, s, pr, uscp, &xJp);
    ctx->cand.ensure(npairs * sizeof(PairRec)); ctx->fullx.ensure(npairs * 4); ctx->fullu.ensure(npairs * 4); ctx->raw.ensure(npairs * 12);
    HIPCHK(hipMemcpyAsync(ctx->cand.p, pr.data(), npairs * sizeof(PairRec), hipMemcpyHostToDevice, ctx->stream));
    std::map<int, std::vector<uint32_t>> vq;
    for (uint32_t i = 0; i < npairs; ++i) vq[p->prof[model[i]].vitQH].push_back(i);
    // queue lengths: the exact-MSV launch, then one per Viterbi register class
    std::vector<uint32_t> qctl(2 + 64, 0u);
    qctl[0] = npairs;
    { size_t k = 1; for (auto &kv : vq) { qctl[k] = (uint32_t)kv.second.size(); ++k; } }
    ctx->vitq.ensure(qctl.size() * 4);
    uint32_t *qd = ctx->vitq.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(qd, qctl.data(), qctl.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    launch_msv_full(ctx->stream, std::min<uint32_t>(npairs, 4096), WorkQueue{nullptr, qd, npairs}, ctx->cand.as<PairRec>(), dm, lt, res, off, dlen,
                    ctx->fullx.as<int32_t>(), ctx->fullu.as<float>(), p->maxMp, nullptr);
    launch_bias(ctx->stream, ctx->cand.as<PairRec>(), npairs, dm, lt, res, off, dlen, ctx->raw.as<float>());
    HIPCHK(hipGetLastError());
    std::vector<int32_t> xJ(npairs); std::vector<float> usc(npairs), raw(npairs * 3);
    HIPCHK(hipMemcpyAsync(xJ.data(), ctx->fullx.p, npairs * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(usc.data(), ctx->fullu.p, npairs * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(raw.data(), ctx->raw.p, npairs * 12, hipMemcpyDeviceToHost, ctx->stream));
    // Viterbi on every pair
    std::vector<uint32_t> flat; std::vector<std::pair<int, std::pair<size_t, size_t>>> vg;
    for (auto &kv : vq) { vg.push_back({kv.first, {flat.size(), kv.second.size()}}); flat.insert(flat.end(), kv.second.begin(), kv.second.end()); }
    ctx->fbidx.ensure(npairs * 4); ctx->vitx.ensure(npairs * 4); ctx->vits.ensure(npairs * 4);
    HIPCHK(hipMemcpyAsync(ctx->fbidx.p, flat.data(), npairs * 4, hipMemcpyHostToDevice, ctx->stream));
    {
      size_t k = 1;
      for (auto &g : vg) {
        const uint32_t cnt = (uint32_t)g.second.second;
        if (launch_vit(g.first, std::min<uint32_t>((cnt + 3) / 4, 2048), ctx->stream, WorkQueue{ctx->fbidx.as<uint32_t>() + g.second.first, qd + k, cnt},
                       ctx->cand.as<PairRec>(), dm, lt, res, off, dlen, ctx->vitx.as<int32_t>(), ctx->vits.as<float>(), nullptr, false, nullptr))
          throw Error(CKM_ERANGE, "no Viterbi kernel instance");
        ++k;
      }
    }
    HIPCHK(hipGetLastError());
    std::vector<int32_t> vx(npairs); std::vector<float> vs(npairs);
    HIPCHK(hipMemcpyAsync(vx.data(), ctx->vitx.p, npairs * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(vs.data(), ctx->vits.p, npairs * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // Forward parser on every pair
    FbBatch fb; uint64_t pos = 0;
    for (uint32_t i = 0; i < npairs; ++i) {
      const int L = s->len[seq[i]];
      FbWork w; memset(&w, 0, sizeof(w));
      w.model = model[i]; w.seq = seq[i]; w.i0 = 0; w.Ld = L; w.Lcfg = L; w.multihit = 1; w.full = 0; w.slot = i;
      w.xs_off = pos; pos += ((uint64_t)(L + 1) * 6 + 31) & ~(uint64_t)31;
      w.aux_off = pos; pos += ((uint64_t)(L + 1) * 3 + 31) & ~(uint64_t)31;
      fb.work.push_back(w);
    }
    ctx->ws.ensure(pos * 4 + 256);
    run_fb(ctx, p, s, fb, true, false, false, nullptr);
    EventIndex ei; ei.build(fb.events, npairs);
    for (uint32_t i = 0; i < npairs; ++i) {
      const int L = s->len[seq[i]];
      const LenEntry &le = s->lentab[L];
      ckm_stage_scores &o = out[i];
      o.ssv_maxv = maxv[i]; o.msv_xJ = xJ[i]; o.msv_sc = usc[i]; o.null_sc = le.nullsc;
      o.msvp_xJ = xJp[i]; o.msvp_sc = uscp[i];
      const float p1 = (float)L / (float)(L + 1);
      const float nullsc = (float)(log((double)raw[(size_t)i * 3]) + (double)raw[(size_t)i * 3 + 1] * kLn2);
      o.bias_sc = nullsc + (float)L * logf(p1) + logf(1.0f - p1);
      o.vit_xC = vx[i]; o.vit_sc = vs[i];
      o.fwd_xC = fb.fout[i].xC; o.fwd_nscale = fb.fout[i].nscale;
      o.fwd_sc = finish_forward(fb.fout[i].xC, le.move_m, ei.scales(i));
    }
  });
}

// The SSV kernel the way the search runs it: ONE model against a list of sequences in the caller's order, blocks of per_block sequences
// built as ckm_search.hip builds them (list_start, count, pair_start; ssv_threads_for(cls) threads), so every wavefront slot, several
// rounds per wavefront, a partly filled last group and several blocks are exercised -- and the fused finish (ssv_finish), which
// ckm_debug_stages never runs.  Two launches: Smax per pair (epi.maxv set), then the product's epilogue with tables sized for every pair.
extern "C" int ckm_debug_ssv(ckm_ctx *ctx_, const ckm_profiles *p, const ckm_seqs *s, uint32_t model, const uint32_t *seq, uint32_t n,
                             uint32_t per_block, int32_t lanes, uint16_t *smax, uint8_t *route, float *usc, int32_t *info) {
  return guarded([&] {
    if (!ctx_ || !p || !s || !seq || !smax || !route || !usc) throw Error(CKM_EINVAL, "NULL argument");
    if (model >= p->hmm.size()) throw Error(CKM_EINVAL, "model index out of range");
    if (p->too_long[model]) throw Error(CKM_ERANGE, "model longer than the instantiated kernel classes");
    if (n == 0 || n > (1u << 24)) throw Error(CKM_EINVAL, "between 1 and 2^24 sequences");
    if (lanes != 0 && lanes != 8 && lanes != 16) throw Error(CKM_EINVAL, "lanes must be 0, 8 or 16");
    std::vector<int64_t> pos_of(s->nseq, -1);
    for (uint32_t i = 0; i < n; ++i) {
      if (seq[i] >= s->nseq) throw Error(CKM_EINVAL, "sequence index out of range");
      if (s->len[seq[i]] <= 0) throw Error(CKM_EINVAL, "empty sequence (the lists of a search hold none)");
      if (pos_of[seq[i]] >= 0) throw Error(CKM_EINVAL, "sequence listed twice");
      pos_of[seq[i]] = i;
    }
    const HostProfile &hp = p->prof[model];
    int cls = ssv_class(hp);
    if (lanes == 8) { if (!hp.ssv8Q) throw Error(CKM_ERANGE, "the model has no 8-lane SSV image"); cls = 100 + hp.ssv8Q; }
    if (lanes == 16) { if (hp.ssvQ > 64) throw Error(CKM_ERANGE, "the model has no 16-lane SSV image"); cls = hp.ssvQ; }
    const uint32_t pb = per_block ? per_block : ssv_per_block(cls);
    const int threads = ssv_threads_for(cls);
    std::vector<SsvBlockWork> work;
    for (uint32_t a = 0; a < n; a += pb) { SsvBlockWork w; w.model = model; w.list_start = a; w.count = std::min(pb, n - a); w.pair_start = a; work.push_back(w); }
    if (info) { info[0] = cls; info[1] = threads; info[2] = (int32_t)pb; info[3] = (int32_t)work.size(); }
    ctx_->settle();
    Worker *ctx = &ctx_->w[0];
    ctx->plan_key.clear();                 // this entry overwrites the worker's SSV tables
    HIPCHK(hipSetDevice(ctx->device));
    const DevModel *dm = p->d_models.as<DevModel>();
    const LenEntry *lt = s->d_lentab.as<LenEntry>();
    const uint8_t *res = s->d_res.as<uint8_t>();
    const uint64_t *off = s->d_off.as<uint64_t>();
    const int32_t *dlen = s->d_len.as<int32_t>();
    ctx->work.ensure(work.size() * sizeof(SsvBlockWork)); ctx->idx.ensure((size_t)n * 4); ctx->maxv.ensure((size_t)n * 2 + 64);
    ctx->surv.ensure((size_t)n * sizeof(PairRec)); ctx->nores.ensure((size_t)n * sizeof(PairRec)); ctx->counters.ensure(64);
    wcopy(ctx, ctx->work.p, work.data(), work.size() * sizeof(SsvBlockWork), hipMemcpyHostToDevice);
    wcopy(ctx, ctx->idx.p, seq, (size_t)n * 4, hipMemcpyHostToDevice);
    HIPCHK(hipMemsetAsync(ctx->maxv.p, 0xff, (size_t)n * 2, ctx->stream));          // 0xffff: "the kernel wrote nothing for this pair"
    HIPCHK(hipMemsetAsync(ctx->counters.p, 0, 64, ctx->stream));
    SsvEpi epi; memset(&epi, 0, sizeof(epi));
    epi.lentab = lt; epi.maxv = ctx->maxv.as<uint16_t>();
    if (launch_ssv(cls, (int)work.size(), threads, ctx->stream, ctx->work.as<SsvBlockWork>(), dm, res, off, dlen, ctx->idx.as<uint32_t>(), epi))
      throw Error(CKM_ERANGE, "no SSV kernel instance");
    const SsvEpi fin{lt, ctx->surv.as<PairRec>(), ctx->counters.as<uint32_t>(), n, ctx->nores.as<PairRec>(), ctx->counters.as<uint32_t>() + 1, n, nullptr};
    if (launch_ssv(cls, (int)work.size(), threads, ctx->stream, ctx->work.as<SsvBlockWork>(), dm, res, off, dlen, ctx->idx.as<uint32_t>(), fin))
      throw Error(CKM_ERANGE, "no SSV kernel instance");
    HIPCHK(hipGetLastError());
    uint32_t cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(smax, ctx->maxv.p, (size_t)n * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(cnt, ctx->counters.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (cnt[0] > n || cnt[1] > n) throw Error(CKM_EHIP, "the SSV finish appended " + std::to_string(cnt[0]) + " survivors and " + std::to_string(cnt[1]) + " exact-kernel pairs for " + std::to_string(n) + " pairs");
    std::vector<PairRec> sv(cnt[0]), nr(cnt[1]);
    if (cnt[0]) wcopy(ctx, sv.data(), ctx->surv.p, (size_t)cnt[0] * sizeof(PairRec), hipMemcpyDeviceToHost);
    if (cnt[1]) wcopy(ctx, nr.data(), ctx->nores.p, (size_t)cnt[1] * sizeof(PairRec), hipMemcpyDeviceToHost);
    for (uint32_t i = 0; i < n; ++i) {
      if (smax[i] == 0xffffu) throw Error(CKM_EHIP, "the SSV kernel wrote no Smax for list entry " + std::to_string(i));
      route[i] = 0; usc[i] = 0.f;
    }
    auto place = [&](const PairRec &r, uint8_t code) {
      if (r.model != model || r.seq >= s->nseq || pos_of[r.seq] < 0) throw Error(CKM_EHIP, "the SSV finish reported a pair that was not listed: model " + std::to_string(r.model) + ", sequence " + std::to_string(r.seq));
      const size_t i = (size_t)pos_of[r.seq];
      if (route[i] != 0) throw Error(CKM_EHIP, "the SSV finish reported list entry " + std::to_string(i) + " twice");
      route[i] = code; usc[i] = r.usc;
    };
    for (const PairRec &r : sv) place(r, 1);
    for (const PairRec &r : nr) place(r, 2);
  });
}

// The filter stages between the MSV stage and Forward the way the device-driven search runs them (ckm_search.hip), on n chosen pairs:
// bias_filter_kernel, vit16_kernel, vit_kernel<QH, true> and the `decide` epilogues, none of which ckm_debug_stages launches.  A private
// CascadeDev for ONE group over the worker's cascade tables, every table sized for all n pairs, the search's margins and grids.
//   VIT16            cand[i] = pair i with the caller's filtersc, the vq of the pairs' one 16-lane class = the caller's order;
//                    vit16_kernel, then vit_kernel<QH, false> with decide on whatever reached vxq (one launch per class present)
//   WAVE_FAST        the same with vit_kernel<QH, true> and decide (legal for short models too: their wave-per-pair class)
//   WAVE_FAST_PLAIN  vit_kernel<QH, true> without decide (out_xC, out_sc, out_flag): the host-driven search's first pass
//   CHAIN            bias_filter_kernel over the candidate table (the caller's usc; classes may mix), then the FAST and the exact
//                    Viterbi kernels of every class present, in the search's order
// Outputs are prefilled with sentinels (all bits set); a queued pair that was not written, a pair reported twice in a queue or as a
// Forward item, and an entry that is no pair of the call are errors (CKM_EHIP) that name the pair.
extern "C" int ckm_debug_filters(ckm_ctx *ctx_, const ckm_profiles *p, const ckm_seqs *s, const uint32_t *model, const uint32_t *seq,
                                 const float *usc, const float *filtersc, uint32_t n, int32_t mode, uint32_t nblocks,
                                 ckm_filter_result *out, uint32_t *status) {
  return guarded([&] {
    if (!ctx_ || !p || !s || !model || !seq || !usc || !out || !status) throw Error(CKM_EINVAL, "NULL argument");
    if (mode < CKM_FILTERS_VIT16 || mode > CKM_FILTERS_CHAIN) throw Error(CKM_EINVAL, "unknown mode");
    if (mode != CKM_FILTERS_CHAIN && !filtersc) throw Error(CKM_EINVAL, "NULL argument");
    if (n == 0 || n > (1u << 22)) throw Error(CKM_EINVAL, "between 1 and 2^22 pairs");
    if (nblocks > 65536) throw Error(CKM_EINVAL, "at most 65536 workgroups");
    const uint32_t nb = nblocks ? nblocks : GRID_VIT;
    bool present[NVC] = {false};
    std::vector<std::vector<uint32_t>> vq(NVC);
    unsigned long long ws_need = 0;
    int q16 = -1;
    for (uint32_t i = 0; i < n; ++i) {
      if (model[i] >= p->hmm.size() || seq[i] >= s->nseq) throw Error(CKM_EINVAL, "pair index out of range");
      if (p->too_long[model[i]]) throw Error(CKM_ERANGE, "model longer than the instantiated kernel classes");
      if (s->len[seq[i]] <= 0) throw Error(CKM_EINVAL, "empty sequence (the lists of a search hold none)");
      const DevModel &d = p->dm[model[i]];
      if (mode == CKM_FILTERS_VIT16) {
        if (!d.vit16Q) throw Error(CKM_ERANGE, "the model has no 16-lane Viterbi image");
        if (q16 >= 0 && q16 != d.vit16Q) throw Error(CKM_EINVAL, "the pairs of a VIT16 call must share one 16-lane class");
        q16 = d.vit16Q;
      }
      const int c = (mode == CKM_FILTERS_VIT16 || mode == CKM_FILTERS_CHAIN) ? d.vit_cls : d.vitx_cls;
      if (c < 0 || c >= NVC || d.vitx_cls < NV16 || d.vitx_cls >= NVC || d.fb_cls < 0 || d.fb_cls >= NFC) throw Error(CKM_ERANGE, "no kernel instance for this model length");
      present[c] = true; present[d.vitx_cls] = true;
      if (mode != CKM_FILTERS_CHAIN) vq[c].push_back(i);
      ws_need += (((unsigned long long)(s->len[seq[i]] + 1) * 6ull) + 31ull) & ~31ull;
    }
    ctx_->settle();
    Worker *ctx = &ctx_->w[0];
    ctx->plan_key.clear();                 // this entry overwrites the worker's cascade tables
    HIPCHK(hipSetDevice(ctx->device));
    const DevModel *dm = p->d_models.as<DevModel>();
    const LenEntry *lt = s->d_lentab.as<LenEntry>();
    const uint8_t *res = s->d_res.as<uint8_t>();
    const uint64_t *off = s->d_off.as<uint64_t>();
    const int32_t *dlen = s->d_len.as<int32_t>();
    hipStream_t st = ctx->stream;
    auto table = [](DevBuf &b, size_t bytes) { b.ensure(std::max<size_t>(64, bytes)); return b.p; };
    uint32_t *d_cnt = (uint32_t *)table(ctx->c_cnt, 2 * CC_SIZE * 4);
    unsigned long long *d_tops = (unsigned long long *)table(ctx->c_tops, 4 * 8);
    CascadeDev cd; memset(&cd, 0, sizeof(cd));
    cd.cand = (PairRec *)table(ctx->c_cand, (size_t)n * sizeof(PairRec)); cd.cap_cand = n;
    cd.bias_raw = (float *)table(ctx->c_bias, (size_t)n * 8);
    cd.vit_fast = (float *)table(ctx->c_vfast, (size_t)n * 4); cd.vit_exact = (float *)table(ctx->c_vexact, (size_t)n * 4);
    cd.vit_flag = (uint32_t *)table(ctx->c_vflag, (size_t)n * 4); cd.route = (uint8_t *)table(ctx->c_route, n);
    cd.vq = (uint32_t *)table(ctx->c_vq, (size_t)n * NVC * 4); cd.vxq = (uint32_t *)table(ctx->c_vxq, (size_t)n * NVC * 4); cd.cap_vq = n;
    cd.fq = (uint32_t *)table(ctx->c_fq, (size_t)n * NFC * 4); cd.cap_fq = n;
    cd.fwork = (FbWork *)table(ctx->c_fwork, (size_t)n * sizeof(FbWork)); cd.cap_fwork = n;
    cd.gcnt = d_cnt; cd.cnt = d_cnt + CC_SIZE;
    cd.ws_top = d_tops; cd.ws_cap = 2 * ws_need;      // (a Forward item only reserves its rows here: nothing of the workspace is touched before Forward)
    cd.seq_len = dlen;
    cd.margin_msv = kMarginMsv; cd.margin_vit = kMarginVit; cd.margin_fwd = kMarginFwd;
    int32_t *d_xC = (int32_t *)table(ctx->vitx, (size_t)n * 4); float *d_sc = (float *)table(ctx->vits, (size_t)n * 4); uint32_t *d_flag = (uint32_t *)table(ctx->vitf, (size_t)n * 4);
    // candidate table, counters, queues
    std::vector<PairRec> pr(n);
    for (uint32_t i = 0; i < n; ++i) { pr[i].model = model[i]; pr[i].seq = seq[i]; pr[i].usc = usc[i]; pr[i].filtersc = mode == CKM_FILTERS_CHAIN ? 0.f : filtersc[i]; }
    std::vector<uint32_t> cnt(2 * CC_SIZE, 0u);
    cnt[CC_SIZE + CC_CAND] = n;
    wcopy(ctx, cd.cand, pr.data(), (size_t)n * sizeof(PairRec), hipMemcpyHostToDevice);
    for (int c = 0; c < NVC; ++c) if (!vq[c].empty()) {
      cnt[CC_SIZE + CC_VQ + c] = (uint32_t)vq[c].size();
      wcopy(ctx, cd.vq + (size_t)c * n, vq[c].data(), vq[c].size() * 4, hipMemcpyHostToDevice);
    }
    wcopy(ctx, d_cnt, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice);
    HIPCHK(hipMemsetAsync(d_tops, 0, 4 * 8, st));
    auto sentinels = [&] {
      HIPCHK(hipMemsetAsync(cd.vit_fast, 0xff, (size_t)n * 4, st)); HIPCHK(hipMemsetAsync(cd.vit_exact, 0xff, (size_t)n * 4, st));
      HIPCHK(hipMemsetAsync(cd.vit_flag, 0xff, (size_t)n * 4, st));
    };
    sentinels();
    HIPCHK(hipMemsetAsync(cd.bias_raw, 0xff, (size_t)n * 8, st));
    HIPCHK(hipMemsetAsync(cd.route, mode == CKM_FILTERS_CHAIN ? 0xee : 1, n, st));      // (0xee: "the bias filter wrote no route"; 1: what it writes for a pair it queues for the FAST kernel)
    HIPCHK(hipMemsetAsync(d_xC, 0xff, (size_t)n * 4, st)); HIPCHK(hipMemsetAsync(d_sc, 0xff, (size_t)n * 4, st)); HIPCHK(hipMemsetAsync(d_flag, 0xff, (size_t)n * 4, st));
    uint32_t *gc = cd.cnt;
    int rc = 0;
    auto exact_launches = [&] {
      for (int c = NVC - 1; c >= NV16; --c) if (present[c])
        rc |= launch_vit(kVitQH[c - NV16], std::max(64u, GRID_VIT / 4), st, WorkQueue{cd.vxq + (size_t)c * cd.cap_vq, gc + CC_VXQ + c, cd.cap_vq}, cd.cand, dm, lt, res, off, dlen, nullptr, nullptr, nullptr, false, &cd);
    };
    if (mode == CKM_FILTERS_CHAIN) {
      launch_bias_filter(st, GRID_MSV, cd, dm, lt, res, off);
      sentinels();                         // (the bias filter zeroes the Viterbi outputs of every candidate: "not written" has to be told from a score again)
    }
    if (mode == CKM_FILTERS_WAVE_FAST_PLAIN) {
      for (int c = NVC - 1; c >= NV16; --c) if (present[c])
        rc |= launch_vit(kVitQH[c - NV16], nb, st, WorkQueue{cd.vq + (size_t)c * cd.cap_vq, gc + CC_VQ + c, cd.cap_vq}, cd.cand, dm, lt, res, off, dlen, d_xC, d_sc, d_flag, true, nullptr);
    } else {
      for (int c = NVC - 1; c >= 0; --c) if (present[c]) {
        const WorkQueue qv{cd.vq + (size_t)c * cd.cap_vq, gc + CC_VQ + c, cd.cap_vq};
        if (c < NV16) rc |= launch_vit16(kVit16Q[c], nb, st, qv, cd.cand, dm, lt, res, off, dlen, cd);
        else rc |= launch_vit(kVitQH[c - NV16], nb, st, qv, cd.cand, dm, lt, res, off, dlen, nullptr, nullptr, nullptr, true, &cd);
      }
      exact_launches();
    }
    if (rc) throw Error(CKM_ERANGE, "no Viterbi kernel instance");
    HIPCHK(hipGetLastError());
    // results
    std::vector<float> raw((size_t)n * 2), vfast(n), vexact(n), psc(n);
    std::vector<uint32_t> vflag(n), pflag(n), lists_vq((size_t)n * NVC), lists_vxq((size_t)n * NVC);
    std::vector<int32_t> pxC(n); std::vector<uint8_t> route(n);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pr.data(), cd.cand, (size_t)n * sizeof(PairRec), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(raw.data(), cd.bias_raw, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(vfast.data(), cd.vit_fast, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(vexact.data(), cd.vit_exact, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(vflag.data(), cd.vit_flag, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(route.data(), cd.route, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(lists_vq.data(), cd.vq, (size_t)n * NVC * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(lists_vxq.data(), cd.vxq, (size_t)n * NVC * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pxC.data(), d_xC, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(psc.data(), d_sc, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pflag.data(), d_flag, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *status = cnt[CC_STATUS];
    const uint32_t nfw = std::min(cnt[CC_FWORK], n);
    std::vector<FbWork> fw(nfw);
    if (nfw) wcopy(ctx, fw.data(), cd.fwork, (size_t)nfw * sizeof(FbWork), hipMemcpyDeviceToHost);
    auto bits_of = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    auto name = [&](uint32_t i) { return "pair " + std::to_string(i) + " (model " + std::to_string(model[i]) + ", sequence " + std::to_string(seq[i]) + ", L = " + std::to_string(s->len[seq[i]]) + ")"; };
    const bool plain = mode == CKM_FILTERS_WAVE_FAST_PLAIN;
    for (uint32_t i = 0; i < n; ++i) {
      ckm_filter_result &o = out[i];
      o.bias_d = raw[2 * (size_t)i]; o.bias_e = raw[2 * (size_t)i + 1]; o.filtersc = pr[i].filtersc;
      o.vit_fast = plain ? psc[i] : vfast[i]; o.vit_exact = vexact[i]; o.vit_flag = plain ? pflag[i] : vflag[i];
      o.vit_xC = plain ? pxC[i] : INT32_MAX; o.route = route[i]; o.n_vq = o.n_vxq = o.n_fwork = 0;
      if (pr[i].model != model[i] || pr[i].seq != seq[i]) throw Error(CKM_EHIP, "the candidate record of " + name(i) + " was overwritten");
    }
    if (cnt[CC_SIZE + CC_CAND] != n) throw Error(CKM_EHIP, "the candidate counter changed");
    for (int c = 0; c < NVC; ++c) {
      const uint32_t nv = cnt[CC_SIZE + CC_VQ + c], nx = cnt[CC_SIZE + CC_VXQ + c];
      if (nv > n || nx > n) throw Error(CKM_EHIP, "queue of class " + std::to_string(c) + " holds " + std::to_string(nv) + " FAST and " + std::to_string(nx) + " exact entries for " + std::to_string(n) + " pairs");
      if ((nv || nx) && !present[c]) throw Error(CKM_EHIP, "entries in the queue of class " + std::to_string(c) + ", which no pair of the call has");
      for (uint32_t k = 0; k < nv; ++k) {
        const uint32_t i = lists_vq[(size_t)c * n + k];
        if (i >= n) throw Error(CKM_EHIP, "FAST queue of class " + std::to_string(c) + ", position " + std::to_string(k) + ": " + std::to_string(i) + " is no pair of the call");
        if (p->dm[model[i]].vit_cls != c && !(mode != CKM_FILTERS_CHAIN && p->dm[model[i]].vitx_cls == c)) throw Error(CKM_EHIP, name(i) + " sits in the FAST queue of class " + std::to_string(c));
        if (out[i].n_vq++) throw Error(CKM_EHIP, name(i) + " sits twice in the FAST queue of class " + std::to_string(c));
        if (bits_of(out[i].vit_fast) == 0xffffffffu || out[i].vit_flag == 0xffffffffu) throw Error(CKM_EHIP, "FAST queue of class " + std::to_string(c) + ", position " + std::to_string(k) + ": the kernel wrote nothing for " + name(i));
      }
      for (uint32_t k = 0; k < nx; ++k) {
        const uint32_t i = lists_vxq[(size_t)c * n + k];
        if (i >= n) throw Error(CKM_EHIP, "exact queue of class " + std::to_string(c) + ", position " + std::to_string(k) + ": " + std::to_string(i) + " is no pair of the call");
        if (p->dm[model[i]].vitx_cls != c) throw Error(CKM_EHIP, name(i) + " sits in the exact queue of class " + std::to_string(c));
        if (out[i].n_vxq++) throw Error(CKM_EHIP, name(i) + " sits twice in the exact queue of class " + std::to_string(c));
        if (bits_of(out[i].vit_exact) == 0xffffffffu) throw Error(CKM_EHIP, "exact queue of class " + std::to_string(c) + ", position " + std::to_string(k) + ": the kernel wrote nothing for " + name(i));
      }
    }
    if (cnt[CC_FWORK] > n) throw Error(CKM_EHIP, std::to_string(cnt[CC_FWORK]) + " Forward items for " + std::to_string(n) + " pairs");
    for (uint32_t t = 0; t < nfw; ++t) {
      const uint32_t i = fw[t].cand;
      if (i >= n || fw[t].model != model[i] || fw[t].seq != seq[i]) throw Error(CKM_EHIP, "Forward item " + std::to_string(t) + " is no pair of the call");
      if (out[i].n_fwork++) throw Error(CKM_EHIP, name(i) + " was handed to Forward twice");
    }
    if (mode == CKM_FILTERS_CHAIN) for (uint32_t i = 0; i < n; ++i) {
      if (out[i].route == 0xee || bits_of(out[i].bias_d) == 0xffffffffu) throw Error(CKM_EHIP, "the bias filter wrote nothing for " + name(i));
    }
  });
}

extern "C" int ckm_debug_envelopes(ckm_ctx *ctx_, const ckm_profiles *p, const ckm_seqs *s, const uint32_t *model, const uint32_t *seq,
                                   const int32_t *ienv, const int32_t *jenv, uint32_t n, ckm_envelope_result *out) {
  return guarded([&] {
    if (!ctx_ || !p || !s || !model || !seq || !ienv || !jenv || !out) throw Error(CKM_EINVAL, "NULL argument");
    ctx_->settle();
    Worker *ctx = &ctx_->w[0];
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<EnvReq> req(n); std::vector<EnvRes> res;
    for (uint32_t i = 0; i < n; ++i) {
      if (model[i] >= p->hmm.size() || seq[i] >= s->nseq || ienv[i] < 1 || jenv[i] > s->len[seq[i]] || jenv[i] < ienv[i]) throw Error(CKM_EINVAL, "bad envelope");
      req[i] = {model[i], seq[i], ienv[i], jenv[i]};
    }
    rescore_envelopes(ctx, p, s, req, res);
    for (uint32_t i = 0; i < n; ++i) {
      out[i].envsc = res[i].envsc; out[i].oasc = res[i].oasc; out[i].fwd_xC = res[i].xC; out[i].nscale = res[i].nscale; out[i].ok = res[i].ok;
      for (int x = 0; x < 20; ++x) out[i].null2[x] = res[i].null2[x];
      out[i].hmm_from = res[i].hmm_from; out[i].hmm_to = res[i].hmm_to; out[i].ali_from = res[i].ali_from; out[i].ali_to = res[i].ali_to;
    }
  });
}

// ckm_debug_envelopes with the OA paths and their posterior lines (rescore_envelopes with paths and pps: the items of
// ckm_hits_write_alignments, whose posterior rows keep a matrix of their own).  out_off[n + 1] / node_residue: int32[M] per item, the
// envelope-local residue of every match node; pp_off[n + 1] / pp: float[Ld + 1] per item.  Both stay zero where ok == 0.
extern "C" int ckm_debug_envelope_paths(ckm_ctx *ctx_, const ckm_profiles *p, const ckm_seqs *s, const uint32_t *model, const uint32_t *seq,
                                        const int32_t *ienv, const int32_t *jenv, uint32_t n, int32_t *ok, const uint64_t *out_off,
                                        int32_t *node_residue, const uint64_t *pp_off, float *pp) {
  return guarded([&] {
    if (!ctx_ || !p || !s || !model || !seq || !ienv || !jenv || !ok || !out_off || !node_residue || !pp_off || !pp) throw Error(CKM_EINVAL, "NULL argument");
    ctx_->settle();
    Worker *ctx = &ctx_->w[0];
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<EnvReq> req(n); std::vector<EnvRes> res;
    for (uint32_t i = 0; i < n; ++i) {
      if (model[i] >= p->hmm.size() || seq[i] >= s->nseq || ienv[i] < 1 || jenv[i] > s->len[seq[i]] || jenv[i] < ienv[i]) throw Error(CKM_EINVAL, "bad envelope");
      if (p->too_long[model[i]]) throw Error(CKM_ERANGE, "model longer than the instantiated kernel classes");
      if (out_off[i + 1] - out_off[i] != (uint64_t)p->hmm[model[i]].M) throw Error(CKM_EINVAL, "out_off does not match the model lengths");
      if (pp_off[i + 1] - pp_off[i] != (uint64_t)(jenv[i] - ienv[i] + 2)) throw Error(CKM_EINVAL, "pp_off does not match the envelope lengths");
      req[i] = {model[i], seq[i], ienv[i], jenv[i]};
    }
    std::vector<std::vector<int32_t>> paths; std::vector<std::vector<float>> pps;
    rescore_envelopes(ctx, p, s, req, res, &paths, &pps);
    for (uint32_t i = 0; i < n; ++i) {
      ok[i] = res[i].ok;
      std::copy(paths[i].begin(), paths[i].end(), node_residue + out_off[i]);
      std::copy(pps[i].begin(), pps[i].end(), pp + pp_off[i]);
    }
  });
}

extern "C" int ckm_debug_region(ckm_ctx *ctx_, const ckm_profiles *p, const ckm_seqs *s, uint32_t model, uint32_t seq, int32_t ireg, int32_t jreg,
                                float *n2sum, int32_t *segs, int32_t *nseg, int32_t cap, int32_t *env, int32_t envcap, int32_t *nenv) {
  return guarded([&] {
    if (!ctx_ || !p || !s || !n2sum || !segs || !nseg || !env || !nenv) throw Error(CKM_EINVAL, "NULL argument");
    if (model >= p->hmm.size() || seq >= s->nseq || ireg < 1 || jreg > s->len[seq] || jreg < ireg) throw Error(CKM_EINVAL, "bad region");
    ctx_->settle();
    Worker *ctx = &ctx_->w[0];
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<RegionReq> req{{model, seq, ireg, jreg}}; std::vector<RegionRes> res;
    run_ensembles(ctx, p, s, req, res);
    const RegionRes &r = res[0];
    for (size_t i = 0; i < r.n2sum.size(); ++i) n2sum[i] = r.n2sum[i];
    for (int t = 0; t < ENS_NSAMPLES; ++t) {
      if (r.nseg[t] > cap) throw Error(CKM_ERANGE, "segment table too small");
      nseg[t] = r.nseg[t];
      for (int d = 0; d < r.nseg[t]; ++d) { const Seg &g = r.segs[(size_t)t * r.cap + d]; int32_t *o = segs + ((size_t)t * cap + d) * 4; o[0] = g.sqfrom; o[1] = g.sqto; o[2] = g.hmmfrom; o[3] = g.hmmto; }
    }
    if ((int)r.env.size() > envcap) throw Error(CKM_ERANGE, "envelope table too small");
    *nenv = (int32_t)r.env.size();
    for (size_t e = 0; e < r.env.size(); ++e) { env[e * 4] = r.env[e].sqfrom; env[e * 4 + 1] = r.env[e].sqto; env[e * 4 + 2] = r.env[e].hmmfrom; env[e * 4 + 3] = r.env[e].hmmto; }
  });
}
