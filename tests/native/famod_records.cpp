// famod_records.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The PTMA prepass of cf_emulator.cpp's emu_spectra_v (prep_famod_a, the warm-start chains, prep_famod_b) on its own,
// returning the fields of the cell records a test needs to know which lanes of k_dndx / k_spectra a surface reaches:
// out[c] = {R_KIND (0: no emission, 1: broken down, 2: modified), R_DET (det B), R_NARROW}.  Built into a library of
// its own (tests/test_gpu_dndx_famod.py); never linked into the product.
#include "cf_emulator.cpp"

extern "C" int emu_famod_records(const orc_params* p, const orc_setup* su, const orc_surface* S, int chains, int op,
                                 double* out) {
  if (p->df_mode != PTMA) return 1;
  const long n = S->n;
  EmuTables et(p, su, op);
  const PrepConsts& k = et.k;
  std::vector<double> rec((size_t)n * NREC), aux((size_t)n * 9), sol((size_t)n * 6);
  const double* fields[NSURF] = {S->tau, S->x, S->y, S->eta, S->dat, S->dax, S->day, S->dan, S->ux, S->uy, S->un,
                                 S->E, S->T, S->P, S->pixx, S->pixy, S->pixn, S->piyy, S->piyn, S->bulkPi,
                                 S->muB, S->nB, S->Vx, S->Vy, S->Vn};
  for (long c = 0; c < n; c++) {
    double s[NSURF];
    for (int f = 0; f < NSURF; f++) s[f] = fields[f] ? fields[f][c] : 0.0;
    prep_famod_a(k, s, &rec[(size_t)c * NREC], &aux[(size_t)c * 9]);
  }
  const int nh = su->npdg < 320 ? su->npdg : 320;
  Hadrons h{nh, su->pdg_mass, su->pdg_sign, su->pdg_degen};
  const double fp2 = 4.0 * pow(M_PI, 2) * pow(kHbarC, 3);
  auto id = [](double v) { return v; };
  const long C = (chains > 0) ? (chains < n ? chains : n) : n;
  for (long ch = 0; ch < C; ch++) {
    double state[4] = {0, 0, 0, 0};
    long cnt[3] = {0, 0, 0};
    for (long c = ch; c < n; c += C) {
      if (rec[(size_t)c * NREC + R_KIND] == 0.0) continue;
      aniso_cell(&aux[(size_t)c * 9], h, 0, 1, id, fp2, state, &sol[(size_t)c * 6], cnt);
    }
  }
  for (long c = 0; c < n; c++) {
    double* R = &rec[(size_t)c * NREC];
    int broken = 0;
    if (R[R_KIND] != 0.0) prep_famod_b(k, R, &aux[(size_t)c * 9], &sol[(size_t)c * 6], &broken);
    out[3 * c] = R[R_KIND];
    out[3 * c + 1] = R[R_KIND] != 0.0 ? R[R_DET] : 0.0;
    out[3 * c + 2] = R[R_KIND] != 0.0 ? R[R_NARROW] : 0.0;
  }
  return 0;
}
