// The readers of tests/cpp/caller.h on their own: no library call is made.
//
//   caller_selftest <dir> keyed|unkeyed [guards]
// reads <dir>/items.txt under the keyed or the unkeyed header and, when asked, <dir>/guards.txt, and prints what it parsed in the
// format it read: the header, a line per proof with its column lengths taken from the parsed columns and its bytes as hex, a line per
// Guard.  tests/test_caller_reader_host.py builds it with the address and undefined-behaviour sanitizers and compares the printout with
// the files; a malformed file must end it with status 2 and nothing printed.
#include <cstring>
#include "caller.h"

using namespace caller;

int main(int argc, char** argv) {
    if (argc < 3 || argc > 4 || (strcmp(argv[2], "keyed") && strcmp(argv[2], "unkeyed")) || (argc == 4 && strcmp(argv[3], "guards"))) {
        fprintf(stderr, "usage: caller_selftest <dir> keyed|unkeyed [guards]\n");
        return 2;
    }
    const std::string d = argv[1];
    const bool keyed = !strcmp(argv[2], "keyed");
    // everything is read before anything is printed
    const Items in = read_items(d, keyed);
    const std::vector<Guard> guards = argc == 4 ? read_guards(d) : std::vector<Guard>();
    if (keyed) printf("%zu ", in.n_keys);
    printf("%zu\n", in.items.size());
    for (const Item& it : in.items) {
        if (keyed) printf("%zu ", it.key);
        printf("%zu", it.inst.size());
        Bytes flat;
        for (const Column& c : it.inst) {
            printf(" %zu", c.size());
            for (const Bytes& v : c) flat.insert(flat.end(), v.begin(), v.end());
        }
        printf(" "); hex_or_dash(it.proof); printf(" "); hex_or_dash(flat); printf("\n");
    }
    for (const Guard& g : guards) {
        hex_or_dash(g.left_scalars); printf(" "); hex_or_dash(g.left_bases); printf(" "); hex_or_dash(g.right_scalars); printf(" "); hex_or_dash(g.right_bases); printf("\n");
    }
    return 0;
}
