// gar_knobs.hpp -- the one reader of the launch planners' environment knob tables (kHxsKnobTable,
// kBgKnobTable, kHxKnobTable).  A table row gives a knob's name, the field it fills (its default: the
// member initialiser of the knob struct), how the value reads and when it is read.  Host only.
#pragma once
#include <cstdlib>

namespace gar {

// atoi of the value; set at all; first character '1'; first character not '0' (unset: on)
enum KnobKind { kInt, kIsSet, kIsOne, kNotZero };
template <class K>
struct KnobRow {
    const char* name;
    int K::*field;
    KnobKind kind;
    bool perLaunch;  // re-read on every launch (tests switch it inside one process), else once per process
};

template <class K, size_t N>
void readKnobTable(const KnobRow<K> (&table)[N], K& k, bool perLaunchOnly) {
    for (const KnobRow<K>& r : table) {
        if (perLaunchOnly && !r.perLaunch) continue;
        const char* e = std::getenv(r.name);
        if (r.kind == kIsSet) k.*r.field = e != nullptr;
        else if (r.kind == kIsOne) k.*r.field = e && e[0] == '1';
        else if (r.kind == kNotZero) k.*r.field = !(e && e[0] == '0');
        else k.*r.field = e ? std::atoi(e) : K{}.*r.field;
    }
}

}  // namespace gar
