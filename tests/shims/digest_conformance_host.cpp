// TEST INFRASTRUCTURE.  Host half of the digest API conformance check (see
// digest_conformance.inl): plain host C++, as a simulator's Manager is.
#define DIGCONF_NAME digconf_host
#include "digest_conformance.inl"
