// Host check of csrc/knobs.h: every parse rule of the header against the expression the call sites spelled out
// before the header existed, over the values a variable can reasonably be given.  Exit code 0: no difference.
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -o knobs_host_check tools/knobs_host_check.cpp
#include <stdio.h>
#include <stdlib.h>

#include "../nodal_amd/csrc/knobs.h"

#define V "NODAL_KNOBS_HOST_CHECK"

static int failures = 0;

template <class A, class B>
static void same(const char *kind, const char *value, A got, B want) {
    if (got == (A)want) return;
    fprintf(stderr, "%s differs for %s\n", kind, value ? value : "(unset)");
    ++failures;
}

int main() {
    const char *values[] = {nullptr, "", "0", "1", "abc", "-3", " 2", "0x10", "1e-3", "-1"};
    for (const char *v : values) {
        if (v) setenv(V, v, 1);
        else unsetenv(V);

        same("Present", v, knob::Present{V}.now(), getenv(V) != nullptr);
        same("OnUnless0", v, knob::OnUnless0{V}.now(), !(getenv(V) && atoi(getenv(V)) == 0));
        same("OffUnlessNon0", v, knob::OffUnlessNon0{V}.now(), getenv(V) && atoi(getenv(V)) != 0);
        // (NODAL_BI_MASKED's inverted rule)
        same("OnIfSet0", v, knob::OnIfSet0{V}.now(), getenv(V) != nullptr && atoi(getenv(V)) == 0);
        {   // (the poison level: unset 0, any set value at least 1)
            int want = 0;
            if (const char *e = getenv(V)) {
                const int x = atoi(e);
                want = x > 1 ? x : 1;
            }
            same("Level", v, knob::Level{V}.now(), want);
            if (v) same("Level, at least 1 when set", v, knob::Level{V}.now() >= 1, true);
        }
        same("Int", v, knob::Int{V, 40}.now(), getenv(V) ? atoi(getenv(V)) : 40);
        same("Int64", v, knob::Int64{V, 20000}.now(), getenv(V) ? atoll(getenv(V)) : (int64_t)20000);
        same("Double", v, knob::Double{V, 16.0}.now(), getenv(V) ? atof(getenv(V)) : 16.0);
        {   // "is it set": the site keeps its own value, or names its own default
            int keep = 7;
            if (const char *e = getenv(V)) keep = atoi(e);
            int got = 7;
            if (const auto x = knob::IntIfSet{V}.now()) got = *x;
            same("IntIfSet", v, got, keep);
            same("Int64IfSet", v, knob::Int64IfSet{V}.now().value_or(5000), getenv(V) ? atoll(getenv(V)) : (int64_t)5000);
            double cap = 0.5;
            if (const char *e = getenv(V)) cap = atof(e) * 1e9;
            double got_cap = 0.5;
            if (const auto gb = knob::DoubleIfSet{V}.now()) got_cap = *gb * 1e9;
            same("DoubleIfSet", v, got_cap, cap);
        }
        same("Text", v, knob::Text{V}.now(), (const char *)getenv(V));
    }
    if (failures) fprintf(stderr, "%d differences\n", failures);
    else printf("knobs: every rule agrees on %d values\n", (int)(sizeof values / sizeof *values));
    return failures ? 1 : 0;
}
