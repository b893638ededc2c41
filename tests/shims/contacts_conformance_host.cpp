// TEST INFRASTRUCTURE.  Host half of the contact query API conformance check
// (see contacts_conformance.inl): plain host C++, as a simulator's Manager is.
#define CONTACTSCONF_NAME contactsconf_host
#include "contacts_conformance.inl"
