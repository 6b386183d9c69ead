// option_text.h -- the "key=value,key=value" texts of the q4_parse_* functions, split in one place. What a key means, whether it may repeat and how its
// value reads stay with each parser.
#pragma once
#include <stddef.h>
#include <string.h>

namespace q4 {

enum { OPTION_KEY_CAP = 32 };

// The pair at *p, copied to key[OPTION_KEY_CAP] and val[val_cap] (both terminated); *p moves behind the pair and its comma. False, with *p where it was:
// no '=', an empty key or value, a key of OPTION_KEY_CAP or a value of val_cap characters or more, a comma with nothing behind it.
static inline bool next_option(const char** p, char* key, char* val, size_t val_cap) {
    const char* s = *p;
    const char* eq = strchr(s, '=');
    const char* end = strchr(s, ',');
    if (!end) end = s + strlen(s);
    if (!eq || eq > end || eq == s || eq + 1 == end) return false;
    const size_t kl = (size_t)(eq - s), vl = (size_t)(end - eq - 1);
    if (kl >= OPTION_KEY_CAP || vl >= val_cap) return false;
    memcpy(key, s, kl); key[kl] = 0;
    memcpy(val, eq + 1, vl); val[vl] = 0;
    if (*end && !end[1]) return false;                         // a trailing comma
    *p = *end ? end + 1 : end;
    return true;
}

}  // namespace q4
