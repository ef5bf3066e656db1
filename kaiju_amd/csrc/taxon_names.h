// taxon_names.h — the host tables of the fourth column (taxon_names.cpp builds them; format_names.hip uploads them;
// tests/emu/format_names_emu.cpp and tests/tools/taxon_names_san.cpp read them).  The C interface is in include/kaiju_gpu.h.
#ifndef KJ_TAXON_NAMES_H
#define KJ_TAXON_NAMES_H

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/kaiju_gpu.h"

// One open-addressing table over the nodes of nodes.dmp as kaiju-addTaxonNames sees them (tax_hash of kj_core.h, linear
// probing, key ~0 = empty; cap is a power of two and at least twice the nodes).
struct kaiju_taxon_names {
  int mode = KAIJU_NAMES_NAME;
  std::vector<uint64_t> key;          // [cap]
  std::vector<uint32_t> parent;       // [cap] slot of the parent (the slot itself: the node is its own parent), kjn::kNone: the parent is no node
  std::vector<uint32_t> name_pos;     // [cap] where the name starts in blob
  std::vector<uint32_t> name_len;     // [cap] bytes of the name; with kjn::kGenerated set: the node has no name and the length is that of "taxonid:<id>"
  std::vector<uint8_t> rank;          // [cap] index of the node's rank in the de-duplicated list, kjn::kNoRank: none (or "no rank")
  std::vector<uint8_t> blob;          // the names one behind the other
  std::vector<std::string> ranks;     // the de-duplicated list
  std::vector<uint8_t> list;          // the list as given: per item the index in `ranks`
  uint64_t n_nodes = 0, n_named = 0;
  // in every mode, for the rows of kaiju2table (host/table_rows.h): the rank of every node as nodes.dmp spells it
  std::vector<std::string> rank_names; // the distinct rank strings, "no rank" among them
  std::vector<uint16_t> rank_of;       // [cap] index in rank_names (empty slots: 0)
  // in every mode, for the lineage lines of kaiju2krona (kj_krona.h): the name of a parent id that is no node.  One per
  // orphan at most, in a blob of their own: no table above changes by them
  std::vector<uint32_t> dang_pos;      // [cap] where the name of the slot's parent id starts in dang_blob
  std::vector<uint32_t> dang_len;      // [cap] its bytes; 0: the parent is a node, or its id has no name; kjn::kNone: a name of 2^24 bytes or more
  std::vector<uint8_t> dang_blob;
};

// what kaiju2krona needs beyond the slot tables on the device: kaiju_gpu_taxon_names_upload keeps a copy on the host, and
// kaiju_gpu_krona_create (krona.hip) makes its tables from it
struct kaiju_krona_source {
  std::vector<std::string> rank_names;
  std::vector<uint16_t> rank_of;
  std::vector<uint32_t> dang_pos, dang_len;
  std::vector<uint8_t> dang_blob;
};

// what a failed call of taxon_names.cpp said (it is also given to kaiju_gpu_last_error() where capi.hip is linked)
extern "C" const char *kaiju_taxon_names_last_error(void);

#endif  // KJ_TAXON_NAMES_H
