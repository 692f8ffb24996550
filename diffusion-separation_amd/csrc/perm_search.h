// perm_search.h — ONE definition of "the source permutation that matches a cross-Gram": r maximises sum_i C[i][r(i)] (= the
// least squared distance between rows i of one signal and rows r(i) of the other), candidates in lexicographic order with a
// strict >, so a tie — two identical rows, an all-silent signal — keeps the earliest maximiser, the identity among them.
// S in 1..3.  Included by longform.hip (neighbouring windows over their overlap) and ensemble.hip (draws against an anchor).
// Free functions only, all __device__ inline in an anonymous namespace.
#pragma once

namespace {

__device__ inline int ds_perm_count(int S) { return S == 3 ? 6 : S; }  // S! for S in 1..3

__device__ inline int ds_perm_entry(int S, int p, int i) {  // entry i of the p-th permutation of 0 .. S - 1, lexicographic
  if (S == 3) {
    const int tab[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    return tab[p][i];
  }
  return S == 2 && p == 1 ? 1 - i : i;
}

// lexicographic index of the permutation r of largest sum_i c[i S + r(i)] (the sum taken i ascending from 0.0)
__device__ inline int ds_best_perm(const double* c, int S) {
  const int nperm = ds_perm_count(S);
  int best = 0;
  double bestv = 0.0;
  for (int q = 0; q < nperm; ++q) {
    double v = 0.0;
    for (int i = 0; i < S; ++i) v += c[i * S + ds_perm_entry(S, q, i)];
    if (q == 0 || v > bestv) { best = q; bestv = v; }
  }
  return best;
}

}  // namespace
