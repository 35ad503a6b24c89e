// Stand-alone host check of mvs::env_int / mvs::env_str (csrc/common.h) against the code they replaced (`e ? atoi(e) : default` on getenv's
// result), for a variable that is unset, empty, non-numeric, negative, a large number and a 4 KB string.  Built with
// AddressSanitizer and UBSan on the host side (there is no device code here) and run by tests/test_abi.py; exits 0 when every case agrees.  Not part of the library.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../mvsformer_amd/csrc/common.h"

static int old_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

int main() {
    const char* name = "MVS_ENV_READER_CHECK";
    const std::string big(4096, '7'), text4k = "12" + std::string(4094, 'x');
    const char* cases[] = {nullptr, "", "abc", "-3", "42", " 7 trailing", "2147483647", "99999999999999999999", big.c_str(), text4k.c_str()};
    int bad = 0;
    for (const char* v : cases) {
        if (v) setenv(name, v, 1);
        else unsetenv(name);
        for (int dflt : {0, 1, 4, 768, 2048}) {
            const int got = mvs::env_int(name, dflt), want = old_int(name, dflt);
            if (got != want) { printf("env_int(%.20s, %d) = %d, the old path gave %d\n", v ? v : "(unset)", dflt, got, want); ++bad; }
        }
        const char* s = mvs::env_str(name);
        if ((s == nullptr) != (v == nullptr) || (s && strcmp(s, v) != 0)) { printf("env_str(%.20s) differs\n", v ? v : "(unset)"); ++bad; }
    }
    // the spot values the knobs rely on
    unsetenv(name);
    bad += mvs::env_int(name, 2048) != 2048;
    setenv(name, "", 1);
    bad += mvs::env_int(name, 4) != 0;
    setenv(name, "abc", 1);
    bad += mvs::env_int(name, 4) != 0;
    setenv(name, "-3", 1);
    bad += mvs::env_int(name, 4) != -3;
    setenv(name, text4k.c_str(), 1);
    bad += mvs::env_int(name, 4) != 12 || strlen(mvs::env_str(name)) != 4096;
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
