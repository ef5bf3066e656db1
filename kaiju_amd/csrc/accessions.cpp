// accessions.cpp — the accession table of an index, host part (needs no GPU): per database sequence the length of its name up
// to its last '_' and the rank of that prefix among the sorted distinct prefixes of the whole index.  Column 6 of kaiju -v is
// the sorted set of the prefixes of a read's matches (ConsumerThread.cpp:822-824, 532); with the ranks the device sorts and
// dedupes at most 20 numbers per read instead of strings (kj_format_verbose.h).
#include <string.h>

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

#include "../../include/kaiju_gpu.h"

// rank[i]: equal prefixes share a rank, ranks are dense from 0 in std::string order (bytes compared as unsigned, a proper prefix
// first); 0xffffffff and prefix_len 0 for a name without '_' (and for a NULL name).  Returns 0 or KAIJU_GPU_ERR_ARG / _NOMEM.
extern "C" int kaiju_accession_ranks(const char *const *names, uint32_t nseq, uint32_t *rank, uint32_t *prefix_len) {
  if (nseq && (!names || !rank || !prefix_len)) return KAIJU_GPU_ERR_ARG;
  try {
    std::vector<uint32_t> order;
    order.reserve(nseq);
    for (uint32_t i = 0; i < nseq; i++) {
      const char *us = names[i] ? strrchr(names[i], '_') : nullptr;
      prefix_len[i] = us ? (uint32_t)(us - names[i]) : 0;
      rank[i] = 0xffffffffu;
      if (us) order.push_back(i);
    }
    auto cmp = [&](uint32_t a, uint32_t b) {              // std::string::compare
      const uint32_t la = prefix_len[a], lb = prefix_len[b];
      const int c = memcmp(names[a], names[b], la < lb ? la : lb);
      return c ? c : (la < lb ? -1 : la > lb ? 1 : 0);
    };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cmp(a, b) < 0; });
    uint32_t next = 0;
    for (size_t k = 0; k < order.size(); k++) {
      if (k && cmp(order[k - 1], order[k]) != 0) next++;
      rank[order[k]] = next;
    }
  } catch (const std::bad_alloc &) { return KAIJU_GPU_ERR_NOMEM; }
  return KAIJU_GPU_OK;
}
