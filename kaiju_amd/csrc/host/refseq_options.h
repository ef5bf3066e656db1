// refseq_options.h — the options of kaiju-convertRefSeq (refseq_main.cpp).  Everything else its host side needs - the readers of
// merged.dmp and of the list of taxa, the cutter - is convert_blocks.h as it is: the tool parses -l and merged.dmp with the
// code of kaiju-convertNR (kaiju-convertRefSeq.cpp:95-135 is kaiju-convertNR.cpp:103-143 line by line).  Plain C++ in a header
// of its own, so that a stand-alone program can drive it under the sanitizers (tests/tools/refseq_options_san.cpp).
#ifndef KJ_REFSEQ_OPTIONS_H
#define KJ_REFSEQ_OPTIONS_H

#include "convert_blocks.h"

namespace kjrs {

// -t nodes.dmp -m merged.dmp -g map -o out [-a] [-l list] [-v] [-d].  The tool's option string is that of kaiju-convertNR,
// "ahdvrm:l:g:t:i:o:e:", but its switch knows neither -i nor -e (nor -r): they end in the usage, as an unknown option does -
// -i and -e with their argument taken, so "-i -t" is one option.  Options::in and Options::excluded stay empty
inline kjcb::Options parse_options(int argc, char **argv) {
  kjcb::Options o;
  optind = 1;
  opterr = 0;
  int c;
  while ((c = getopt(argc, argv, "ahdvrm:l:g:t:i:o:e:")) != -1) {
    switch (c) {
      case 'h': o.help = true; return o;
      case 'd': o.debug = true; break;
      case 'v': o.verbose = true; break;
      case 'a': o.add_acc = true; break;
      case 'l': o.list = optarg; break;
      case 'm': o.merged = optarg; break;
      case 't': o.nodes = optarg; break;
      case 'g': o.map = optarg; break;
      case 'o': o.out = optarg; break;
      default: o.bad_option = true; return o;
    }
  }
  // the order and the words of kaiju-convertRefSeq.cpp:72-75
  if (o.nodes.empty()) o.error = "Please specify the location of the nodes.dmp file, using the -t option.";
  else if (o.merged.empty()) o.error = "Please specify the location of the merged.dmp file, using the -m option.";
  else if (o.map.empty()) o.error = "Please specify the location of the prot.accession2taxid file, using the -g option.";
  else if (o.out.empty()) o.error = "Please specify the name of the output file, using the -o option.";
  return o;
}

}  // namespace kjrs

#endif  // KJ_REFSEQ_OPTIONS_H
